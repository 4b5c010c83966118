#!/usr/bin/env python
"""What the continuum rows of an opacity database cost: 198 temperatures x 5 CIA pairs (H2H2 first) on a synthetic CIA table
of 1 000 knots, onto uniform grids of 1e5 and 1e6 points between 300 and 30 000 cm-1 (smoothing windows of 305 and 3 031
points over regions of 4 208 and 42 087).  The two data tables are synthetic, of the real ones' shapes.

  (a) device   ``of.continuum_rows`` over chunks of temperatures of at most 1 GiB, the rows left on the device
  (b) host     ``of.continuum_rows_numpy`` on one host core for HOST_TEMPS temperatures (one below 600 K), scaled to 198
  (c) filter   the device timer around ``picaso_continuum_rows_dev`` for one chunk with and without the median filter: the
               difference is the filter alone (copy aside and selection), scaled to 198 temperatures

One JSON line per grid size."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import opacity_factory as of            # noqa: E402
from picaso_amd.device import DeviceArray, sync, timer_start, timer_stop          # noqa: E402

NTEMP, PAIRS = 198, ["H2H2", "H2He", "H2H", "H2CH4", "H2N2"]
BUDGET = 1 << 30


def world():
    rng = np.random.default_rng(1460)
    temps = np.concatenate((np.linspace(75.0, 590.0, 40), np.linspace(600.0, 4000.0, NTEMP - 40)))
    old_wno = np.arange(0.0, 20000.0, 20.0)
    og = -6.0 - 1e-4 * old_wno[None, None, :] + rng.uniform(-1.0, 1.0, (NTEMP, len(PAIRS), old_wno.size))
    og[:, 0, old_wno > 9000] = -33.0
    og[:, :, 0] = -33.0
    wn = np.arange(11000.0, 16400.0, 10.0)
    ov = (wn, np.array([60., 80., 100., 150., 200., 250., 300., 350.]), 10.0 ** rng.uniform(-18, -11, (wn.size, 8)))
    lam = np.geomspace(151883.0, 3505.0, 18)
    bell = (np.array([0.5, 0.8, 1.0, 1.2, 1.6, 2.0, 2.8, 3.6, 10.0]), lam, 10.0 ** rng.uniform(-2, 2, (9, 18)))
    return temps, old_wno, og, ov, bell


def main():
    temps, old_wno, og, ov, bell = world()
    host_temps = int(os.environ.get("HOST_TEMPS", "3"))
    reps = int(os.environ.get("REPS", "3"))
    for nwno in [int(x) for x in os.environ.get("NWNO", "100000,1000000").split(",")]:
        new_wno = np.linspace(300.0, 30000.0, nwno)
        per = max(1, BUDGET // (8 * (len(PAIRS) + 3) * nwno))
        res = {"nwno": nwno, "ntemp": NTEMP, "npairs": len(PAIRS), "window": of.smoothing_window(new_wno),
               "region": int(np.sum((new_wno > 9950) & (new_wno < 11200))), "temps_per_chunk": per}

        def device():
            for t0 in range(0, NTEMP, per):
                of.continuum_rows(og[t0:t0 + per], temps[t0:t0 + per], old_wno, PAIRS, new_wno, ov, bell, out="device").free()

        device()                                        # warm-up
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            device()
            times.append(1e3 * (time.perf_counter() - t0))
        res["device_ms"] = round(statistics.median(times), 2)

        pick = np.linspace(0, NTEMP - 1, host_temps).astype(int)
        t0 = time.perf_counter()
        of.continuum_rows_numpy(og[pick], temps[pick], old_wno, PAIRS, new_wno, ov, bell)
        res["host_ms_scaled"] = round(1e3 * (time.perf_counter() - t0) * NTEMP / host_temps, 1)
        res["host_temps_timed"] = host_temps

        n = min(per, NTEMP - 40)
        timed = {}
        for smooth in (False, True):
            dev = of._ContinuumDevice(og[40:40 + n], temps[40:40 + n], old_wno, PAIRS, new_wno, ov, bell, smooth, 0)
            d_out, d_work = DeviceArray((n, dev.nsp, nwno), dev.ctx), dev.work(n)
            dev.rows(0, n, d_out, d_work)
            sync(dev.ctx)
            ts = []
            for _ in range(reps):
                timer_start(dev.ctx)
                dev.rows(0, n, d_out, d_work)
                ts.append(timer_stop(dev.ctx))
            timed[smooth] = statistics.median(ts)
            dev.free()
            d_out.free()
            d_work.free()
        res["kernels_ms_scaled"] = round(timed[True] * NTEMP / n, 3)
        res["filter_ms_scaled"] = round((timed[True] - timed[False]) * NTEMP / n, 3)
        res["device_below_host"] = bool(res["device_ms"] < res["host_ms_scaled"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
