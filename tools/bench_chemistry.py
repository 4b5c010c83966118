#!/usr/bin/env python
"""What equilibrium chemistry from a table costs on the device against the host numpy it replaces (GPU only; one JSON line).

Shape: one native GCM map, 128 x 64 columns x 53 levels = 434 176 points x the 50 species of a 2121-point Visscher grid
(tests/golden/chemistry.npz holds one).  Measured in one run:

  kernel        the device timer around ``picaso_chem_interp_dev`` on resident points, abundances (``10**x``) and exponents
                (``log10=True``): the write of npoints x nspecies x 8 bytes = 174 MB is its floor, so the achieved bytes per
                second of that write are reported beside the time;
  batch         ``chemistry.chem_interp_batch`` from host arrays to host arrays: log10 P on the host, two uploads, the
                launch, the copy back of the 174 MB and the split into per-species arrays;
  chemeq_3d     ``inputs.premix_3d`` (the body of ``chemeq_3d`` behind its file read) on 10 x 10 facets x 53 levels;
  numpy         ``chemistry.interp_numpy`` on the same points.

Per device figure the median of REPS repetitions, each ending in a blocking copy or a device timer read."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib, chemistry, device      # noqa: E402
from picaso_amd import justdoit as jdi              # noqa: E402
from picaso_amd.device import DeviceArray           # noqa: E402

REPS = int(os.environ.get("CHEM_BENCH_REPS", "9"))
NLON, NLAT, NLEVEL = 128, 64, 53


def median_ms(fn, reps=REPS):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "chemistry.npz"))
    table = {str(k): gold["t2121/%s" % k] for k in gold["t2121/columns"]}
    rng = np.random.default_rng(1)
    pressure = np.broadcast_to(np.logspace(-6, 2, NLEVEL)[:, None, None], (NLEVEL, NLON, NLAT))
    temperature = (600.0 + 1400.0 * np.linspace(0, 1, NLEVEL))[:, None, None] * (1.0 + 0.3 * rng.uniform(-1, 1, (1, NLON, NLAT)))
    npoints = temperature.size
    ctx = _lib.context()
    tab = chemistry.ChemTable.resident(table, ctx)
    out_bytes = npoints * tab.nspecies * 8
    d_t = DeviceArray.from_host(temperature.reshape(-1), ctx)
    d_p = DeviceArray.from_host(np.log10(pressure).reshape(-1), ctx)
    res = {"shape": [NLON, NLAT, NLEVEL], "npoints": npoints, "nspecies": tab.nspecies, "output_MB": out_bytes / 1e6, "reps": REPS}
    for name, log10 in (("kernel_ms", False), ("kernel_log10_ms", True)):
        chemistry.chem_interp_dev(tab, d_t, d_p, npoints, None, log10)
        times = []
        for _ in range(REPS):
            device.timer_start(ctx)
            out = chemistry.chem_interp_dev(tab, d_t, d_p, npoints, None, log10)
            times.append(device.timer_stop(ctx))
            del out
        res[name] = statistics.median(times)
    res["kernel_write_GBps"] = out_bytes / res["kernel_ms"] / 1e6
    res["batch_ms"] = median_ms(lambda: chemistry.chem_interp_batch(temperature, pressure, tab))
    res["batch_GBps"] = out_bytes / res["batch_ms"] / 1e6
    d_out = chemistry.chem_interp_dev(tab, d_t, d_p, npoints, None, False)
    res["copy_back_ms"] = median_ms(d_out.to_host)                       # the floor of the host-to-host call on this box
    case = jdi.inputs()
    case.phase_angle(0.0, num_gangle=10, num_tangle=10)
    case.atmosphere_3d({"pressure": pressure[:, 0, 0], "temperature": temperature[:, :10, :10]})
    opa = type("Opa", (), {"full_abunds": table})()
    res["chemeq_3d_10x10x53_ms"] = median_ms(lambda: case.premix_3d(opa))
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        _, host = chemistry.interp_numpy(temperature.reshape(-1), pressure.reshape(-1), table)
    res["numpy_ms"] = (time.perf_counter() - t0) * 1e3
    got = chemistry.chem_interp_batch(temperature, pressure, tab)
    worst = max(float(np.max(np.abs(got[sp].reshape(-1) - host[:, i]) / np.spacing(host[:, i]))) for i, sp in enumerate(tab.species))
    res["worst_ulp_vs_numpy"] = worst
    res["speedup_batch_vs_numpy"] = res["numpy_ms"] / res["batch_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
