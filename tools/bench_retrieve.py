#!/usr/bin/env python
"""What one proposal of a free retrieval costs from the cube to the log-likelihood through ``retrieve.log_likelihood``,
against the same rows one at a time and against the way before (GPU only; one JSON line).

Shape: S = 1 000 proposals on 90 layers, at 12 500 and at 1e5 wavelengths of synthetic resident opacity tables, thermal,
``pt_knots`` + ``chem_free`` + one grey slab; two instruments, 400 binned points and 400 Gaussian points at R = 100.
Measured in one run, per sample:

  batched          (a) ``log_likelihood(cubes)``, all S rows in one call;
  one_at_a_time    (b) the same function one row per call, over the first SUB rows;
  before           (c) the way before this module, over the first SUBC rows: per sample ``setup_spectrum_class`` ->
                   ``spectrum()`` at full resolution, host ``mean_regrid`` and ``conv_non_uniform_R`` per instrument, the numpy
                   likelihood -- the parent's own public calls;
  reduce           (d) ``picaso_instruments_reduce_dev`` alone against the two member launches
                   (``picaso_mean_regrid_dev`` + ``picaso_lsf_convolve_dev``) by the device timer, one thermal row.

Per figure the median of REPS repetitions with the smallest and the largest beside it."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib, device                  # noqa: E402
from picaso_amd import justdoit as jdi              # noqa: E402
from picaso_amd import optics as px                 # noqa: E402
from picaso_amd import parameterizations as pz      # noqa: E402
from picaso_amd import regrid as rg                 # noqa: E402
from picaso_amd import retrieve as rt               # noqa: E402

REPS = int(os.environ.get("RETRIEVE_BENCH_REPS", "5"))
S = int(os.environ.get("RETRIEVE_BENCH_SAMPLES", "1000"))
SUB = int(os.environ.get("RETRIEVE_BENCH_SINGLE", "32"))
SUBC = int(os.environ.get("RETRIEVE_BENCH_BEFORE", "8"))
GRIDS = [int(x) for x in os.environ.get("RETRIEVE_BENCH_NWNO", "12500,100000").split(",")]
NLEVEL, NIN, NPOINTS = 91, 196, 400


def stats_ms(fn, reps=REPS, per=1):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3 / per)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def opacities(ctx, nwno):
    """Synthetic resident tables (the ones of tools/bench_clouds4d.py) on ``nwno`` wavenumbers."""
    wno = np.linspace(2000.0, 33333.0, nwno)
    temps, press = [100.0, 300.0, 700.0, 1500.0, 3000.0], [1e-6, 1e-4, 1e-2, 1e-1, 1.0, 10.0, 100.0, 500.0]
    pt = [(i + 1, p, t) for i, (t, p) in enumerate((t, p) for t in temps for p in press)]
    mols = ["H2O", "CH4", "CO", "NH3", "H2"]
    molecular = {m: {i: 10.0 ** (-24.0 + 2.0 * np.sin(wno / 2500.0 + k) + 0.4 * np.log10(p) + 0.8 * np.log10(t / 300.0))
                     for (i, p, t) in pt} for k, m in enumerate(mols)}
    cia_t = [75.0, 200.0, 500.0, 1000.0, 2000.0, 4000.0]
    continuum = {pr: {t: 10.0 ** (-7.0 + np.cos(wno / 4000.0 + k) + 0.3 * np.log10(t / 300.0)) for t in cia_t}
                 for k, pr in enumerate(("H2H2", "H2He"))}
    ray = {m: 1e-27 * (wno / 1e4) ** 4 for m in ("H2", "He")}
    return px.RetrieveOpacities(wno, pt, molecular, continuum, cia_t, rayleigh_opa=ray, query_method="linear", ctx=ctx)


def cloud_grid(wno):
    """A $picaso_refdata whose wave_EGP.dat is a 196-point grid inside the opacity grid."""
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "opacities"))
    grid = np.round(np.geomspace(wno[0] * 1.01, wno[-1] * 0.99, NIN), 2)
    with open(os.path.join(d, "opacities", "wave_EGP.dat"), "w") as fh:
        fh.write("   i   wavenumber\n")
        for i, w in enumerate(grid[::-1]):
            fh.write("%4d %.2f\n" % (i + 1, w))
    os.environ["picaso_refdata"] = d


def configuration(wno):
    names = ("k1", "k2", "k3", "k4")
    lo, hi = (300.0, 500.0, 800.0, 1000.0), (400.0, 600.0, 900.0, 1200.0)
    uniform = lambda a, b, log=False: {"prior": "uniform", "log": log, "uniform_kwargs": {"min": a, "max": b}}
    rng = np.random.default_rng(11)
    binned = np.linspace(wno[0] * 1.05, wno[-1] * 0.95, NPOINTS)
    prism = np.linspace(0.32, 4.9, NPOINTS)
    return {
        "calc_type": "retrieval", "observation_type": "thermal", "irradiated": False,
        "geometry": {"phase": {"value": 0.0, "unit": "radian"}},
        "object": {"radius": {"value": 1.0, "unit": "Rjup"}, "mass": {"value": 1.0, "unit": "Mjup"},
                   "distance": {"value": 10.0, "unit": "parsec"}},
        "temperature": {"profile": "knots",
                        "pressure": {"min": {"value": 1e-6, "unit": "bar"}, "max": {"value": 1e2, "unit": "bar"},
                                     "nlevel": NLEVEL, "spacing": "log"},
                        "knots": {"P_knots": {k: {"value": p} for k, p in zip(names, (1e-6, 1e-3, 1.0, 1e2))},
                                  "T_knots": {k: {"value": 0.5 * (a + b)} for k, a, b in zip(names, lo, hi)},
                                  "interpolation": "brewster"}},
        "chemistry": {"method": "free", "free": {"H2O": {"value": 1e-3}, "CH4": {"value": 5e-4},
                                                 "background": {"gases": ["H2", "He"], "fraction": 5.6}}},
        "clouds": {"c1_type": "brewster_grey", "c1": {"brewster_grey": dict(
            decay_type="slab", alpha=0, ssa=0.8, reference_wave=1, slab_kwargs=dict(ptop=-3.0, dp=1.0, reference_tau=0.5))}},
        "InputOutput": {"observation_data": {
            "binned": {"wavelength": 1e4 / binned, "y": 1e-20 * (1.0 + rng.random(NPOINTS)), "e": np.full(NPOINTS, 2e-21)},
            "prism": {"wavelength": prism, "y": 1e-20 * (1.0 + rng.random(NPOINTS)), "e": np.full(NPOINTS, 2e-21), "R": 100.0}}},
        "retrieval": {"temperature": {"knots": {"T_knots": {k: uniform(a, b) for k, a, b in zip(names, lo, hi)}}},
                      "chemistry": {"free": {"H2O": uniform(-4.0, -2.5, log=True)}},
                      "offset": {"prism": uniform(-1e-21, 1e-21)}, "err_inf": {"binned": uniform(-44.0, -41.0, log=True)}},
    }


def before(config, fitpars, data, opa, param, row):
    """One proposal the way before: the full-resolution spectrum, the host reductions, the numpy likelihood."""
    cfg = rt._copy_config(config)
    keys = list(fitpars)
    for i, key in enumerate(keys):
        if not key.startswith(("offset", "scaling", "err_inf")):
            rt.set_dict_value(cfg, key + ".value", row[i])
    out = rt.setup_spectrum_class(cfg, opa, param).spectrum(opa, calculation="thermal")
    flux = rt._flux_scale(cfg) * out["thermal"]
    ymod = [jdi.mean_regrid(out["wavenumber"], flux, newx=data["binned"][0])[1],
            jdi.conv_non_uniform_R(flux, 1e4 / out["wavenumber"], data["prism"][3], 1e4 / data["prism"][0])]
    ydat = [data["binned"][1], data["prism"][1] + row[keys.index("offset.prism")]]
    sigma = [data["binned"][2] ** 2 + row[keys.index("err_inf.binned")], data["prism"][2] ** 2]
    ydat, ymod, sigma = (np.concatenate(x) for x in (ydat, ymod, sigma))
    return -0.5 * np.sum((ydat - ymod) ** 2 / sigma + np.log(2 * np.pi * sigma))


def reduce_alone(ctx, opa, plan):
    """(d): the one call against the two member launches on one resident thermal row, by the device timer (ms)."""
    lib = _lib.load()
    rng = np.random.default_rng(2)
    d_v = device.DeviceArray.from_host(1e6 * rng.random(opa.nwno), ctx)
    row = (rg._Row * 1)()
    row[0].op, row[0].a = 0, d_v.addr
    out = device.DeviceArray((plan.nout,), ctx)
    mean, gauss = plan.members["binned"], plan.members["prism"]

    def timed(fn):
        times = []
        for _ in range(REPS + 1):
            device.timer_start(ctx)
            fn()
            times.append(device.timer_stop(ctx))
        return {"median_ms": statistics.median(times[1:]), "min_ms": min(times[1:]), "max_ms": max(times[1:])}

    def members():
        mean.launch(ctx, 1, row, out.addr)
        gauss.launch(ctx, 1, row, out.addr + 8 * mean.nout)
    one = timed(lambda: plan.launch(ctx, 1, row, out.addr))
    got = out.to_host()
    two = timed(members)
    return {"instruments_reduce": one, "member_launches": two,
            "equal": bool(np.array_equal(got, out.to_host(), equal_nan=True))}


def main():
    ctx = _lib.context()
    res = {"samples": S, "single_rows": SUB, "before_rows": SUBC, "nlayer": NLEVEL - 1, "points_per_instrument": NPOINTS,
           "reps": REPS, "grids": {}}
    for nwno in GRIDS:
        opa = opacities(ctx, nwno)
        cloud_grid(opa.wno)
        config = configuration(opa.wno)
        param = pz.Parameterize()
        data = rt.get_data(config)
        loglike, prior, fitpars = rt.make_loglike(config, opa, data, param)
        cube = prior(np.random.default_rng(7).random((S, len(fitpars))))
        r = {}
        batched = loglike(cube)
        r["batched"] = stats_ms(lambda: loglike(cube), per=S)
        r["one_at_a_time"] = stats_ms(lambda: [loglike(row) for row in cube[:SUB]], per=SUB)
        r["before"] = stats_ms(lambda: [before(config, fitpars, data, opa, param, row) for row in cube[:SUBC]], per=SUBC)
        single = np.array([loglike(row) for row in cube[:SUB]])
        old = np.array([before(config, fitpars, data, opa, param, row) for row in cube[:SUBC]])
        r["rows_equal_batch"] = bool(np.array_equal(single, batched[:SUB]))
        r["worst_relative_distance_from_before"] = float(np.max(np.abs(old - batched[:SUBC]) / np.abs(old)))
        r["reduce"] = reduce_alone(ctx, opa, rg.instruments_plan(opa, rt._instruments(config, data)))
        res["grids"][str(nwno)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
