#!/usr/bin/env python
"""What the prediction bands of a retrieval cost on the device against the host sorts they replace (GPU only; one JSON line).

  bands         ``retrieval.bands`` of 1 000 draws x 20 000 columns and of 1 000 x 100 000, the reference's seven lines:
                the kernel alone (device timer around ``picaso_column_quantiles_dev`` on a resident matrix), the whole
                call on a resident matrix (launch + the copy of the (7, N) result), and the whole call on a host array
                (the upload of the matrix added).
  bands_batch   ``analyze.bands_batch`` of 1 000 samples between the nodes of tools/bench_gridfit.py's 4-parameter grid
                (625 models x 20 000 wavelengths): interpolation, bands, copy of (7, 20 000); and binned to its 100 data
                points.
  host          in the same run, the host way: seven ``get_line`` calls, each a sort of every column, by a numpy
                restatement of ``scipy.stats.mstats.mquantiles`` (``np.apply_along_axis`` of sort-and-blend, as scipy
                does it); at 100 000 columns one line is timed and multiplied by seven.

Per device figure the median of REPS repetitions, each ending in a blocking copy or a device timer read.
BANDS_PROFILE=1: 20 calls of each device path and nothing else, for ``rocprofv3 --kernel-trace --stats -- python
tools/bench_bands.py`` (row k_column_quantiles)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from picaso_amd import _lib, analyze, device, retrieval      # noqa: E402
from picaso_amd.device import DeviceArray                    # noqa: E402
import bench_gridfit                                         # noqa: E402

NDRAWS = 1000
LEVELS = list(retrieval.SIGMA_QUANTILES.values())


def host_get_line(ys, q, alphap=0.4, betap=0.4):
    """``mquantiles(ys, q, axis=0)[0]`` as scipy computes it: per column, in a Python loop, sort and blend."""
    p = np.atleast_1d(np.asarray(q, dtype=float))
    m = alphap + p * (1. - alphap - betap)

    def one(col):
        x = np.sort(col)
        n = len(x)
        aleph = (n * p + m)
        k = np.floor(aleph.clip(1, n - 1)).astype(int)
        gamma = (aleph - k).clip(0, 1)
        return (1. - gamma) * x[(k - 1).tolist()] + gamma * x[k.tolist()]
    return np.apply_along_axis(one, 0, ys)[0]


def kernel_ms(d, k, gamma, reps):
    ctx = d.ctx
    out = []
    for _ in range(reps):
        device.sync(ctx)
        device.timer_start(ctx)
        res = retrieval.column_quantiles(d, k, gamma)
        out.append(device.timer_stop(ctx))
        res.free()
    return round(statistics.median(out), 3)


def main():
    reps = int(os.environ.get("REPS", "7"))
    profile = bool(os.environ.get("BANDS_PROFILE"))
    ctx = _lib.context(0)
    rng = np.random.default_rng(5)
    res = {"draws": NDRAWS, "levels": len(LEVELS), "reps": reps}
    k, gamma = retrieval.quantile_table(NDRAWS, LEVELS)

    wl4, spectra4, gp4, data4 = bench_gridfit.world((5, 5, 5, 5), 2)
    f4 = analyze.GridFitter("g", wavelength=wl4, spectra=spectra4, grid_params=gp4, verbose=False)
    f4.add_data("d", *data4)
    f4.prep_gridtrieval("g")
    pars = list(f4.interp_params["g"]["grid_parameters_unique"].values())
    goals = np.stack([a[0] + np.random.default_rng(3 + p).random(NDRAWS) * (a[-1] - a[0]) for p, a in enumerate(pars)],
                     axis=1)
    analyze.bands_batch(goals, f4, "g")                      # warm-up: code objects, staging, the pool's blocks
    analyze.bands_batch(goals, f4, "g", data_name="d")

    for ncol in (20000, 100000):
        ys = 0.01 + 0.001 * rng.standard_normal((NDRAWS, ncol))
        d = DeviceArray.from_host(ys, ctx)
        got = retrieval.bands(d)
        if profile:
            for _ in range(20):
                retrieval.bands(d)
            continue
        row = {"kernel_ms": kernel_ms(d, k, gamma, reps),
               "call_resident_ms": bench_gridfit.median_ms(lambda: retrieval.bands(d), reps),
               "call_with_upload_ms": bench_gridfit.median_ms(lambda: retrieval.bands(ys), reps),
               "matrix_mb": round(ys.nbytes / 1e6, 1)}
        t0 = time.perf_counter()
        if ncol <= 20000:
            want = np.stack([host_get_line(ys, q) for q in LEVELS])
            row["host_seven_lines_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            row["equal_to_host"] = bool(np.array_equal(got, want))
        else:
            want = host_get_line(ys, 0.5)
            row["host_seven_lines_ms"] = round(7e3 * (time.perf_counter() - t0), 1)
            row["host_lines_timed"] = 1
            row["equal_to_host"] = bool(np.array_equal(got[6], want))
        res["bands_%d" % ncol] = row
        d.free()
    if profile:
        for _ in range(20):
            analyze.bands_batch(goals, f4, "g")
        return

    res["bands_batch"] = {"samples": NDRAWS, "models": spectra4.shape[0], "parameters": 4, "nwave": bench_gridfit.NWAVE,
                          "full_ms": bench_gridfit.median_ms(lambda: analyze.bands_batch(goals, f4, "g"), reps),
                          "binned_ms": bench_gridfit.median_ms(lambda: analyze.bands_batch(goals, f4, "g", data_name="d"),
                                                               reps)}
    t0 = time.perf_counter()
    stack = analyze.interp_batch(goals, f4, "g")
    t1 = time.perf_counter()
    want = np.stack([host_get_line(stack, q) for q in LEVELS])
    res["bands_batch"]["interp_batch_copy_back_ms"] = round(1e3 * (t1 - t0), 1)
    res["bands_batch"]["host_seven_lines_ms"] = round(1e3 * (time.perf_counter() - t1), 1)
    res["bands_batch"]["equal_to_host"] = bool(np.array_equal(analyze.bands_batch(goals, f4, "g"), want))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
