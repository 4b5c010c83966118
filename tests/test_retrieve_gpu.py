"""``instruments=`` on the public calls and ``retrieve.MODEL`` / ``log_likelihood`` on the GPU, on the synthetic database of
tests/test_optics.py.

Among the device's own results the criterion is bit identity: a slice of ``spectrum(instruments=...)`` is the array of
``spectrum(regrid=...)`` / ``spectrum(convolve=...)``, and a row of a cube is the row alone, whatever ``N`` and the batch
size.  Against the plain route written out here (``setup_spectrum_class`` -> ``spectrum()`` -> host ``mean_regrid`` /
``conv_non_uniform_R`` of ``k * thermal``) the binned instrument is bit for bit and the Gaussian one is held to
tests/test_convolve_host.py's bound plus one unit of ``2^-53`` for the product.  The clouds of that comparison are grey with
``alpha = 0``, where the table made in HBM has the host table's bits (tests/test_parameterize_gpu.py)."""
import copy
import os
import shutil

import numpy as np
import pytest

from mie_cases import synthetic_table
from test_chemistry_host import DIR_2121
from test_convolve_host import bound
from test_optics import DB
from test_parameterize_gpu import _case, _cloud_grid

pytestmark = pytest.mark.gpu

SPECTRAL = ("albedo", "fpfs_reflected", "thermal", "fpfs_thermal", "fpfs_total", "transit_depth")
NEWX = np.linspace(5000.0, 24000.0, 6)
WL, R = np.array([0.5, 2.2, 0.8, 1.5]), np.array([30.0, 15.0, 20.0, 25.0])
INS = {"a": {"newx": NEWX}, "b": {"wl": WL, "R": R}}
RJUP, MJUP, PARSEC = 7.1492e9, 1.8981246e30, 3.0856775814913674e18


@pytest.fixture(scope="module")
def og():
    from helpers import GOLDEN
    return np.load(os.path.join(GOLDEN, "optics.npz"))


@pytest.fixture(scope="module")
def opa():
    from picaso_amd import justdoit as jdi
    return jdi.opannection(filename_db=DB, query_method="linear")


@pytest.fixture(scope="module")
def refdata(tmp_path_factory, og):
    """``$picaso_refdata`` for the module: a 67-point cloud grid inside the opacity grid and the synthetic 2121 grid."""
    root = tmp_path_factory.mktemp("refdata")
    mp = pytest.MonkeyPatch()
    _cloud_grid(root, mp, og)
    shutil.copytree(DIR_2121, str(root / "chemistry" / "visscher_grid_2121"))
    yield root
    mp.undo()


def same_slices(got, a, b, tag):
    """``got`` (instruments=) against ``a`` (regrid=) and ``b`` (convolve=): key by key, bit for bit."""
    keys = list(a)
    assert list(got) == [("instrument_counts" if k == "regrid_counts" else k) for k in keys] + ["instrument_slices"], tag
    assert list(b) == [("convolve_counts" if k == "regrid_counts" else k) for k in keys], tag
    sl = got["instrument_slices"]
    assert list(sl) == ["a", "b"] and (sl["a"], sl["b"]) == (slice(0, 6), slice(6, 10))
    n = 0
    for k in keys:
        if k == "wavenumber" or k in SPECTRAL and isinstance(a[k], np.ndarray):
            assert got[k].shape == (10,), (tag, k)
            assert np.array_equal(got[k][sl["a"]], a[k], equal_nan=True), (tag, k)
            assert np.array_equal(got[k][sl["b"]], b[k], equal_nan=True), (tag, k)
            n += 1
        elif k == "regrid_counts":
            assert np.array_equal(got["instrument_counts"], np.concatenate([a[k], b["convolve_counts"]]))
        else:
            assert np.array_equal(got[k], a[k]) and np.array_equal(got[k], b[k]), (tag, k)
    return n


def test_instruments_keyword_against_regrid_and_convolve(og, opa, refdata):
    from picaso_amd import justdoit as jdi
    calc = "reflected+thermal"
    plain_before = _case(og).spectrum(opa, calculation=calc)
    a = _case(og).spectrum(opa, calculation=calc, regrid=INS["a"])
    b = _case(og).spectrum(opa, calculation=calc, convolve=INS["b"])
    got = _case(og).spectrum(opa, calculation=calc, instruments=INS)
    assert same_slices(got, a, b, "spectrum") == 6 and np.all(np.isfinite(got["thermal"]))
    same_slices(_case(og).spectrum_async(opa, calculation=calc, instruments=INS).result(), a, b, "async")
    plan = jdi.instruments_plan(opa, INS)
    same_slices(jdi.picaso(_case(og), opa, calculation=calc, instruments=plan), a, b, "picaso, a plan")
    # full_output goes through the Spectrum path; the spectral arrays are the same
    full = _case(og).spectrum(opa, calculation=calc, instruments=INS, full_output=True)
    assert all(np.array_equal(full[k], got[k], equal_nan=True) for k in SPECTRAL if k in got)
    # every member of a batch (3 members, 2 per launch), each against its own calls
    cases = lambda: [_case(og, k=k) for k in range(3)]
    batch = jdi.spectrum_batch(cases(), opa, calculation=calc, batch_size=2, instruments=INS)
    for k, out in enumerate(batch):
        same_slices(out, _case(og, k=k).spectrum(opa, calculation=calc, regrid=INS["a"]),
                    _case(og, k=k).spectrum(opa, calculation=calc, convolve=INS["b"]), "batch %d" % k)
    assert not np.array_equal(batch[0]["thermal"], batch[2]["thermal"])
    # one plan per case: a scale on the second only
    per_case = jdi.spectrum_batch(cases()[:2], opa, calculation=calc, instruments=[plan, plan.with_scale(0.5)])
    assert np.array_equal(per_case[0]["thermal"], batch[0]["thermal"], equal_nan=True)
    assert np.array_equal(per_case[1]["thermal"][:6], 0.5 * batch[1]["thermal"][:6], equal_nan=True)       # a power of two: exact
    # a call without the keyword: the dictionary it returned before, keys and bits
    plain_after = _case(og).spectrum(opa, calculation=calc)
    assert list(plain_after) == list(plain_before) and "instrument_slices" not in plain_after
    assert all(np.array_equal(plain_after[k], plain_before[k]) for k in plain_before)
    assert list(_case(og).spectrum(opa, calculation="nothing", instruments=INS)) == ["wavenumber", "instrument_counts",
                                                                                     "instrument_slices"]
    with pytest.raises(NotImplementedError, match="instruments= with devices=N"):
        _case(og).spectrum(opa, calculation=calc, instruments=INS, devices=2)
    with pytest.raises(Exception, match="give one of them"):
        _case(og).spectrum(opa, calculation=calc, instruments=INS, regrid={"R": 20.0})


# ------------------------------------------------------------------------------------------------------ MODEL, log_likelihood
def make_config(chem="free", cloud="brewster_grey", cold=False, table=None):
    t_lo = (76.0, 80.0, 88.0, 95.0) if cold else (300.0, 500.0, 800.0, 1000.0)
    t_hi = (79.0, 86.0, 94.0, 99.0) if cold else (400.0, 600.0, 900.0, 1200.0)
    names = ("k1", "k2", "k3", "k4")
    uniform = lambda lo, hi, log=False: {"prior": "uniform", "log": log, "uniform_kwargs": {"min": lo, "max": hi}}
    config = {
        "calc_type": "retrieval", "observation_type": "thermal", "irradiated": False,
        "geometry": {"phase": {"value": 0.0, "unit": "radian"}},
        "object": {"radius": {"value": 1.0, "unit": "Rjup"}, "mass": {"value": 1.0, "unit": "Mjup"},
                   "distance": {"value": 10.0, "unit": "parsec"}},
        "temperature": {"profile": "knots",
                        "pressure": {"min": {"value": 1e-4, "unit": "bar"}, "max": {"value": 10.0, "unit": "bar"}, "nlevel": 12,
                                     "spacing": "log"},
                        "knots": {"P_knots": {k: {"value": p} for k, p in zip(names, (1e-4, 1e-2, 1.0, 10.0))},
                                  "T_knots": {k: {"value": 0.5 * (lo + hi)} for k, lo, hi in zip(names, t_lo, t_hi)},
                                  "interpolation": "brewster"}},
        "InputOutput": {"observation_data": {
            "nirspec": {"wavelength": 1e4 / np.array([20000.0, 5000.0, 8750.0, 12500.0, 16250.0]),
                        "y": 1e-20 * np.array([1.0, 3.0, 2.5, 2.0, 1.5]), "e": np.full(5, 2e-21)},
            "prism": {"wavelength": WL, "y": 1e-20 * np.array([0.8, 2.9, 1.1, 2.2]), "e": np.full(4, 3e-21), "R": R}}},
        "retrieval": {"temperature": {"knots": {"T_knots": {k: uniform(lo, hi) for k, lo, hi in zip(names, t_lo, t_hi)}}},
                      "sampler": {"resume": False},
                      "offset": {"prism": uniform(-1e-21, 1e-21)}, "scaling": {"nirspec": uniform(0.8, 1.2)},
                      "err_inf": {"nirspec": uniform(-44.0, -41.0, log=True)}},
    }
    if chem == "free":
        config["chemistry"] = {"method": "free", "free": {"H2O": {"value": 1e-3}, "CH4": {"value": 3e-4},
                                                          "background": {"gases": ["H2", "He"], "fraction": 5.6}}}
        config["retrieval"]["chemistry"] = {"free": {"H2O": uniform(-4.0, -2.5, log=True)}}
    else:
        config["chemistry"] = {"method": "visscher", "visscher": {"cto_absolute": {"value": 0.55}, "log_mh": 0.0}}
        config["retrieval"]["chemistry"] = {"visscher": {"cto_absolute": uniform(0.2, 0.6)}}
    if cloud == "brewster_grey":
        config["clouds"] = {"c1_type": "brewster_grey", "c1": {"brewster_grey": dict(
            decay_type="slab", alpha=0, ssa=0.8, reference_wave=1, slab_kwargs=dict(ptop=-2.75, dp=1.5, reference_tau=0.5))}}
    elif cloud == "flex_fsed":
        config["clouds"] = {"c1_type": "flex_fsed", "c1": {"flex_fsed": dict(
            table=table, base_pressure=0.5, ndz=3e5, fsed=0.7, distribution="lognorm",
            lognorm_kwargs={"sigma": 0.3, "lograd": -4.1})}}
    return config


def same_tree(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    return type(a) is type(b) and (a is b or a == b)


def unit_cube(ndim):
    u = np.random.default_rng(5).random((5, ndim))
    u[0], u[1] = 0.1, 0.9
    return u


def expression(config, fitpars, data, row, model):
    """The reference's likelihood expression (driver.py:286-326) for one row, written out."""
    keys = list(fitpars)
    ydat, ymod, sig = [], [], []
    for name in config["InputOutput"]["observation_data"]:
        off = row[keys.index("offset." + name)] if name in config["retrieval"].get("offset", {}) else 0
        scl = row[keys.index("scaling." + name)] if name in config["retrieval"].get("scaling", {}) else 1
        inf = row[keys.index("err_inf." + name)] if name in config["retrieval"].get("err_inf", {}) else 0
        ydat.append((data[name][1] + off) * scl), ymod.append(model[name]), sig.append(data[name][2] ** 2 + inf)
    ydat, ymod, sig = (np.concatenate(x) for x in (ydat, ymod, sig))
    return -0.5 * np.sum((ydat - ymod) ** 2 / sig + np.log(2 * np.pi * sig))


def run_rows(config, opa):
    """``MODEL`` and ``log_likelihood`` for five rows at once and one at a time: the checks every variant shares."""
    from picaso_amd import retrieve as rt
    from picaso_amd.parameterizations import Parameterize
    p = Parameterize()
    data = rt.get_data(config)
    loglike, prior, fitpars = rt.make_loglike(config, opa, data, p)
    cube = prior(unit_cube(len(fitpars)))
    kept = copy.deepcopy({k: v for k, v in config.items() if k != "clouds"}), dict(config.get("clouds", {}))
    models, profiles = rt.MODEL(cube, fitpars, config, opa, p, data, retrieval=False)
    logl = loglike(cube)
    assert same_tree({k: v for k, v in config.items() if k != "clouds"}, kept[0])          # the caller's config is as it was
    assert config.get("clouds", {}) == kept[1]
    assert logl.shape == (5,) and list(models) == ["nirspec", "prism"]
    assert models["nirspec"].shape == (5, 5) and models["prism"].shape == (5, 4)
    for j in range(5):
        one = rt.MODEL(cube[j], fitpars, config, opa, p, data)
        for name in models:
            assert one[name].shape == (1, models[name].shape[1])
            assert np.array_equal(one[name][0], models[name][j], equal_nan=True), (j, name)
        alone = loglike(cube[j])
        assert np.shape(alone) == () and np.array_equal(alone, logl[j], equal_nan=True), j
        want = expression(config, fitpars, data, cube[j], {k: v[j] for k, v in models.items()})
        assert np.array_equal(logl[j], want, equal_nan=True), j
    assert not np.array_equal(models["nirspec"][0], models["nirspec"][1])                  # the rows differ
    return p, data, fitpars, cube, models, profiles, logl


def test_model_rows_do_not_depend_on_the_batch_and_equal_the_plain_route(og, opa, refdata):
    from picaso_amd import justdoit as jdi
    from picaso_amd import parameterizations as pz
    from picaso_amd import retrieve as rt
    config = make_config()
    launches = pz.LAUNCHES
    p, data, fitpars, cube, models, profiles, logl = run_rows(config, opa)
    # MODEL (5 rows), loglike (5 rows), then per row one MODEL and one loglike: one cloud launch each
    assert pz.LAUNCHES == launches + 2 + 2 * 5
    before = pz.LAUNCHES
    rt.log_likelihood(cube, fitpars, config, opa, data, p)
    assert pz.LAUNCHES == before + 1                                   # five proposals, one launch
    assert np.all(np.isfinite(logl)) and all(np.all(np.isfinite(m)) and np.all(m > 0) for m in models.values())
    assert profiles[3]["temperature"].shape == (12,) and "H2O" in profiles[3].keys()
    k = 1e-8 * ((1.0 * RJUP) / (10.0 * PARSEC)) ** 2
    prism = jdi.convolve_plan(opa, 1e4 / data["prism"][0], data["prism"][3])
    for j, row in enumerate(cube):
        cfg = copy.deepcopy(config)
        for i, key in enumerate(fitpars):
            if not key.startswith(("offset", "scaling", "err_inf")):
                assert rt.set_dict_value(cfg, key + ".value", row[i])
        case = rt.setup_spectrum_class(cfg, opa, p)
        h2o = row[list(fitpars).index("chemistry.free.H2O")]
        assert case.nlevel == 12 and np.array_equal(case.inputs["atmosphere"]["profile"]["H2O"], np.full(12, h2o))
        out = case.spectrum(opa, calculation="thermal")
        flux = k * out["thermal"]
        binned = jdi.mean_regrid(out["wavenumber"], flux, newx=data["nirspec"][0])[1]
        assert np.array_equal(models["nirspec"][j], binned), j
        ref = jdi.conv_non_uniform_R(flux, 1e4 / out["wavenumber"], data["prism"][3], 1e4 / data["prism"][0])
        mag = jdi.conv_non_uniform_R(np.abs(flux), 1e4 / out["wavenumber"], data["prism"][3], 1e4 / data["prism"][0])
        lim = bound(prism.counts, mag) + 2.0 ** -53 * mag
        err = np.abs(models["prism"][j] - ref)
        print("row %d: Gaussian instrument, worst |out - ref| / bound %.3f" % (j, float(np.max(err / lim))))
        assert np.all(err <= lim), j
    with pytest.raises(NotImplementedError, match="defines no reflected branch"):
        rt.MODEL(cube, fitpars, dict(config, observation_type="reflected"), opa, p, data)


def test_visscher_rows_share_one_launch_per_grid_file(og, opa, refdata, monkeypatch):
    from picaso_amd import chemistry as ch
    config = make_config(chem="visscher", cold=True)
    calls = []
    real = ch.chem_interp_batch
    monkeypatch.setattr(ch, "chem_interp_batch", lambda t, p, table, **kw: (calls.append(np.shape(t)), real(t, p, table, **kw))[1])
    p, data, fitpars, cube, models, profiles, logl = run_rows(config, opa)
    cto = cube[:, list(fitpars).index("chemistry.visscher.cto_absolute")]
    files = [os.path.basename(ch.select_visscher_2121(c, 0.0)) for c in cto]
    assert len(set(files)) == 2                                        # two grid files in one batch
    sizes = sorted(files.count(f) for f in set(files))
    assert sorted(calls[:2]) == [(sizes[0], 12), (sizes[1], 12)] and sorted(calls[2:4]) == sorted(calls[:2])
    assert all(c == (1, 12) for c in calls[4:]) and len(calls) == 4 + 2 * 5
    print("visscher: log-likelihoods", logl)
    for j in range(5):
        prof = profiles[j]
        table = ch.visscher_2121(cto[j], 0.0)
        species, x = ch.interp_numpy(prof["temperature"], prof["pressure"], table, log10=True)
        assert len(species) == 50 and all(s in prof.keys() for s in species)
        for i, sp in enumerate(species):
            assert np.max(np.abs(prof[sp] - 10.0 ** x[:, i]) / np.spacing(10.0 ** x[:, i])) <= 4.0, (j, sp)


def test_mie_decks_take_one_launch_per_call(og, opa, refdata):
    from picaso_amd import mie
    from picaso_amd import retrieve as rt
    wno = og["in/wno"]
    table = synthetic_table(67, 1, seed=4, lo_um=1e4 / (wno.max() * 0.97), hi_um=1e4 / (wno.min() * 1.02))
    config = make_config(cloud="flex_fsed", table=table)
    launches = mie.LAUNCHES
    p, data, fitpars, cube, models, profiles, logl = run_rows(config, opa)
    assert mie.LAUNCHES == launches + 2 + 2 * 5
    before = mie.LAUNCHES
    again = rt.log_likelihood(cube, fitpars, config, opa, data, p)
    assert mie.LAUNCHES == before + 1 and np.array_equal(again, logl)
    assert np.all(np.isfinite(logl))
    clear = make_config(cloud=None)
    free = rt.MODEL(cube, fitpars, clear, opa, p, data)
    assert not np.array_equal(free["nirspec"], models["nirspec"])        # the cloud is seen


def test_transmission_rows_are_the_transit_depth_of_regrid_and_convolve(og, opa, refdata, tmp_path):
    """``observation_type = 'transmission'`` (an irradiated planet with a star from a file): no flux scale, so a row is the
    ``transit_depth`` of ``spectrum(regrid=...)`` and of ``spectrum(convolve=...)`` bit for bit."""
    from picaso_amd import retrieve as rt
    wl = np.linspace(0.3, 3.0, 400)
    np.savetxt(tmp_path / "star.txt", np.stack([wl, 1e14 * (1.0 + 0.3 * np.sin(5.0 * wl)) / wl ** 4], axis=1))
    # a planet keeps the default raman='pollack' (the reference's driver sets no approx()), which reads this table
    np.savetxt(refdata / "opacities" / "raman_fortran.txt", np.stack([wl, 1.0 - 0.02 / wl], axis=1))
    config = make_config(cloud=None)
    config.update(observation_type="transmission", irradiated=True,
                  star={"type": "userfile", "userfile": {"filename": str(tmp_path / "star.txt"), "w_unit": "um",
                                                         "f_unit": "erg/cm2/s/cm"},
                        "radius": {"value": 1.0, "unit": "Rsun"}, "semi_major": {"value": 0.05, "unit": "AU"}})
    for name in config["InputOutput"]["observation_data"]:
        obs = config["InputOutput"]["observation_data"][name]
        obs["y"], obs["e"] = 0.011 + 0.0 * obs["y"], 1e-4 + 0.0 * obs["e"]
    config["retrieval"]["offset"]["prism"]["uniform_kwargs"] = {"min": -1e-4, "max": 1e-4}
    config["retrieval"]["err_inf"]["nirspec"]["uniform_kwargs"] = {"min": -9.0, "max": -8.0}
    p, data, fitpars, cube, models, profiles, logl = run_rows(config, opa)
    assert np.all(np.isfinite(logl)) and np.all(models["nirspec"] > 0) and np.all(models["nirspec"] < 1)
    for j in (0, 3):
        cfg = copy.deepcopy(config)
        for i, key in enumerate(fitpars):
            if not key.startswith(("offset", "scaling", "err_inf")):
                assert rt.set_dict_value(cfg, key + ".value", cube[j][i])
        a = rt.setup_spectrum_class(cfg, opa, p).spectrum(opa, calculation="transmission", regrid={"newx": data["nirspec"][0]})
        b = rt.setup_spectrum_class(cfg, opa, p).spectrum(
            opa, calculation="transmission", convolve={"wl": 1e4 / data["prism"][0], "R": data["prism"][3]})
        assert np.array_equal(models["nirspec"][j], a["transit_depth"]) and np.array_equal(models["prism"][j], b["transit_depth"])
