#!/usr/bin/env python
"""What fitting a model grid costs on the device against the host loops it replaces (GPU only; one JSON line).

  fit_grid       1 000 models x 20 000 wavelengths against 100 data points: ``GridFitter.fit_grid`` INCLUDING the upload of
                 the spectra (a fresh fitter per repetition), against the reference's loop -- ``jdi.mean_regrid`` per
                 model, the mean offset, ``chi_squared`` -- on the host in the same run.  Also ``fit_grid`` alone on a
                 fitter whose spectra are resident.
  loglike_batch  S = 1 024 samples between the nodes of a 4-parameter grid (5 x 5 x 5 x 5 = 625 models x 20 000
                 wavelengths), binned to the same 100 data points, against a numpy restatement of the reference's
                 per-sample loop (the 16-corner sum of ``custom_interp``, ``mean_regrid``, the likelihood expression).

Per figure the median of REPS repetitions, each ending in a blocking copy of the result.  The bytes a sample must read are
``2^d * nwave * 8``; ``loglike_gb_per_call`` is that times S.  GRIDFIT_PROFILE=1: 20 calls of each device path and nothing
else, for ``rocprofv3 --kernel-trace --stats -- python tools/bench_gridfit.py`` (rows k_grid_rows_binned, k_grid_loglike)."""
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib, analyze             # noqa: E402
from picaso_amd import justdoit as jdi           # noqa: E402

NWAVE, NDATA = 20000, 100


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3)


def world(shape, seed):
    """A square grid of ``prod(shape)`` smooth spectra with noise, its parameters, and 100 data points."""
    rng = np.random.default_rng(seed)
    wl = np.linspace(0.6, 5.3, NWAVE)
    nodes = [np.linspace(0.0, 1.0, n) + 0.01 * np.arange(n) ** 2 for n in shape]
    cols = np.array(list(itertools.product(*nodes)))
    base = 0.01 + 0.001 * np.sin(3.0 * wl)
    spectra = base[None, :] * (1.0 + 0.1 * cols @ rng.random(len(shape))[:, None]) + 1e-5 * rng.random((cols.shape[0], NWAVE))
    gp = {"planet_params": {"p%d" % p: cols[:, p] for p in range(len(shape))}}
    cen = np.linspace(1.0, 5.0, NDATA)
    y = np.interp(cen, wl, base) * 1.05 + 1e-5 * rng.standard_normal(NDATA)
    e = 2e-5 * (0.5 + rng.random(NDATA))
    return wl, spectra, gp, (cen, np.gradient(cen), y, e)


def host_fit_grid(wl, spectra, cen, y, e):
    chi2 = np.empty(spectra.shape[0])
    for i in range(spectra.shape[0]):
        m = jdi.mean_regrid(wl, spectra[i], newx=cen)[1]
        chi2[i] = analyze.chi_squared(y, e, m + np.mean(y - m), 0)
    return chi2


def host_loglike(goals, pars, square, wl, cen, y, e):
    """The reference's per-sample loop: custom_interp's corner sum, mean_regrid, driver.py:326."""
    out = np.empty(len(goals))
    for s, goal in enumerate(goals):
        lo = [analyze.find_bounding_values(a, v) for a, v in zip(pars, goal)]
        w = np.array([(v - b[0][0]) / (b[0][1] - b[0][0]) for b, v in zip(lo, goal)])
        aw = np.array([1 - w, w]).T
        interp = 0
        for bits in itertools.product([0, 1], repeat=len(pars)):
            inds = [b[1][j] for b, j in zip(lo, bits)] + [-1]
            interp += np.prod([aw[i][j] for i, j in enumerate(bits)]) * analyze.get_last_dimension(square, inds)
        m = jdi.mean_regrid(wl, interp, newx=cen)[1]
        sigma = e ** 2
        out[s] = -0.5 * np.sum((y - m) ** 2 / sigma + np.log(2 * np.pi * sigma))
    return out


def main():
    reps = int(os.environ.get("REPS", "7"))
    profile = bool(os.environ.get("GRIDFIT_PROFILE"))
    _lib.context(0)
    res = {"nwave": NWAVE, "ndata": NDATA, "reps": reps}

    wl, spectra, gp, data = world((10, 10, 10), 1)

    def fresh():
        f = analyze.GridFitter("g", wavelength=wl, spectra=spectra, grid_params=gp, verbose=False)
        f.add_data("d", *data)
        return f

    def with_upload():
        f = fresh()
        f.fit_grid("g", "d")
        return f

    resident = with_upload()                      # warm-up: code objects, pinned staging, the pool's blocks
    wl4, spectra4, gp4, data4 = world((5, 5, 5, 5), 2)
    f4 = analyze.GridFitter("g", wavelength=wl4, spectra=spectra4, grid_params=gp4, verbose=False)
    f4.add_data("d", *data4)
    f4.prep_gridtrieval("g")
    S = int(os.environ.get("SAMPLES", "1024"))
    pars = list(f4.interp_params["g"]["grid_parameters_unique"].values())
    goals = np.stack([a[0] + np.random.default_rng(3 + p).random(S) * (a[-1] - a[0]) for p, a in enumerate(pars)], axis=1)
    logl = analyze.loglike_batch(goals, f4, "g", "d")
    if profile:
        for _ in range(20):
            resident.fit_grid("g", "d")
            analyze.loglike_batch(goals, f4, "g", "d")
        return

    res["fit_grid"] = {"models": spectra.shape[0],
                       "device_with_upload_ms": median_ms(with_upload, reps),
                       "device_resident_ms": median_ms(lambda: resident.fit_grid("g", "d"), reps)}
    t0 = time.perf_counter()
    chi2 = host_fit_grid(wl, spectra, data[0], data[2], data[3])
    res["fit_grid"]["host_loop_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["fit_grid"]["max_rel_diff_chi2"] = float(np.max(np.abs(resident.chi_sqs["g"]["d"] - chi2) / chi2))
    res["fit_grid"]["same_rank"] = bool(np.array_equal(resident.rank["g"]["d"], chi2.argsort()))

    res["loglike_batch"] = {"samples": S, "models": spectra4.shape[0], "parameters": 4,
                            "device_ms": median_ms(lambda: analyze.loglike_batch(goals, f4, "g", "d"), reps),
                            "gb_per_call": round(S * 16 * NWAVE * 8 / 1e9, 3)}
    nhost = min(S, int(os.environ.get("HOST_SAMPLES", "128")))
    square = f4.interp_params["g"]["square_spectra_grid"]
    t0 = time.perf_counter()
    want = host_loglike(goals[:nhost], pars, square, wl4, data4[0], data4[2], data4[3])
    per = (time.perf_counter() - t0) / nhost
    res["loglike_batch"]["host_loop_ms"] = round(1e3 * per * S, 1)
    res["loglike_batch"]["host_samples_timed"] = nhost
    res["loglike_batch"]["max_rel_diff"] = float(np.max(np.abs(logl[:nhost] - want) / np.abs(want)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
