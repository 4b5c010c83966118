#!/usr/bin/env python
"""What ``jdi.photon_attenuation`` costs at 1e5 wavelengths x 90 layers (monochromatic resident synthetic opacity tables,
the atmosphere of tools/bench_regrid.py with a cloud deck on a 196-point grid of its own), on an MI355X:

  case_ms        ``jdi.photon_attenuation(case, opa)``: planes formed on the device, 3 x nwno pressures and 4 x nwno ints back
  dict_ms        ``jdi.photon_attenuation(full_output)``: the four planes uploaded first
  k_tau_level_ms the kernel alone on resident planes (device timer)
  copy_4_planes_ms  the four (nlayer, nwno) planes copied to the host, which is what the reference's function needs first
  host_loop_ms   a numpy restatement of the reference's per-column np.unique / argmin loop (justplotit.py:848-859, three
                 components) on one host core, on HOST_COLS columns (default: all) and scaled to nwno when fewer

Host clock around calls that end in a copy to the host (so the stream has drained), medians over BLOCKS blocks of the
mean of CALLS calls after a warm-up; the kernel by the device timer around CALLS launches.  ``bytes`` is what the kernel
must move -- four planes read once, three pressure rows and four int rows written -- and ``k_tau_level_GBps`` that over
the kernel time: the figure the byte count is judged against.  No time is a requirement.  One JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_regrid import world                   # noqa: E402
from picaso_amd import _lib, device, optics       # noqa: E402
from picaso_amd import justdoit as jdi           # noqa: E402
from picaso_amd.attenuation import _tau_levels   # noqa: E402
from picaso_amd.contribution import _case_planes  # noqa: E402
from picaso_amd.device import DeviceArray        # noqa: E402


def cloudy_world():
    case, opa = world(int(os.environ.get("NWNO", "100000")))
    nlayer, grid = 90, np.linspace(opa.wno.min(), opa.wno.max(), 196)
    x = (grid - grid[0]) / (grid[-1] - grid[0])
    deck = np.zeros((nlayer, 1))
    deck[55:70] = 0.3
    case.clouds(df={"opd": (deck * (0.5 + x)[None, :]).ravel(), "w0": np.tile(0.6 + 0.39 * x, nlayer),
                    "g0": np.tile(0.8 - 0.3 * x, nlayer)}, wavenumber=grid)
    return case, opa


def median_ms(fn, nblocks, calls):
    out = []
    for _ in range(nblocks):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return round(statistics.median(out), 4)


def host_levels(planes, at_tau, cols):
    """The reference's loop: per column and component np.unique of the cumulative column, the first minimum of
    |value - at_tau|, the last level that holds that value."""
    out = np.zeros((3, cols), dtype=np.int32)
    for k, d in enumerate(planes):
        cum = np.zeros((d.shape[0] + 1, cols))
        cum[1:] = np.cumsum(d[:, :cols], axis=0)
        for w in range(cols):
            vals, first, count = np.unique(cum[:, w], return_index=True, return_counts=True)
            i = np.abs(vals - at_tau).argmin()
            out[k, w] = first[i] + count[i] - 1
    return out


def main():
    nblocks, calls = int(os.environ.get("BLOCKS", "7")), int(os.environ.get("CALLS", "10"))
    at_tau = 0.5
    case, opa = cloudy_world()
    ctx, nwno = opa.ctx, opa.nwno
    res = {"nwno": nwno, "nlayer": 90, "at_tau": at_tau, "blocks": nblocks, "calls_per_block": calls}
    got = jdi.photon_attenuation(case, opa, at_tau=at_tau)                       # warm-up of the case form
    full = case.spectrum(opa, calculation="thermal", full_output=True)["full_output"]
    same = jdi.photon_attenuation(full, at_tau=at_tau)                          # ... and of the dictionary form
    res["case_equals_dict"] = bool(all(np.array_equal(got[k], same[k], equal_nan=True) for k in got))
    res["case_ms"] = median_ms(lambda: jdi.photon_attenuation(case, opa, at_tau=at_tau), nblocks, calls)
    res["dict_ms"] = median_ms(lambda: jdi.photon_attenuation(full, at_tau=at_tau), nblocks, max(1, calls // 5))
    # the kernel alone, on resident planes
    atm, (taugas, taucld, tauray), _, _, _ = _case_planes(case, opa, "1d")
    w0 = optics._cloud_opd_device(atm, opa, key="w0")
    nlayer = atm.c.nlayer
    mono = (nwno, 1, 0)
    comps = [(taugas, mono, None, None), (taucld, mono, w0, mono), (tauray, mono, None, None)]
    plevel = np.asarray(atm.level["pressure"], dtype=float) / atm.c.pconv
    levels, _ = _tau_levels(ctx, nlayer, nwno, comps, plevel, at_tau)
    lib = _lib.load()
    table, layout = _lib.ptr_array([c[0] for c in comps] + [None, w0, None]), np.array([mono] * 6, dtype=np.int64)
    d_lev, d_p, plev = DeviceArray((2 * nwno,), ctx), DeviceArray((3, nwno), ctx), _lib.f64(plevel)

    def kernel():
        _lib.check(lib.picaso_tau_level_dev(ctx, nlayer, nwno, table, layout.ctypes.data, _lib.ptr(plev), 0, at_tau, 0,
                                            d_lev.addr, _lib.ptr(d_p.addr)), ctx)
    kernel()
    device.sync(ctx)
    times = []
    for _ in range(nblocks):
        device.timer_start(ctx)
        for _ in range(calls):
            kernel()
        times.append(device.timer_stop(ctx) / calls)
    res["k_tau_level_ms"] = round(statistics.median(times), 4)
    res["bytes"] = 4 * nlayer * nwno * 8 + 3 * nwno * 8 + 4 * nwno * 4
    res["k_tau_level_GBps"] = round(res["bytes"] / (res["k_tau_level_ms"] * 1e-3) / 1e9, 1)
    planes = (taugas, taucld, w0, tauray)
    res["copy_4_planes_ms"] = median_ms(lambda: [p.to_host() for p in planes], nblocks, max(1, calls // 5))
    # the reference's way on the host, after that copy
    g, c, w, r = (p.to_host() for p in planes)
    cols = min(nwno, int(os.environ.get("HOST_COLS", str(nwno))))
    t0 = time.perf_counter()
    ref = host_levels((g, c * w, r), at_tau, cols)
    host = 1e3 * (time.perf_counter() - t0)
    res["host_cols"] = cols
    res["host_loop_ms"] = round(host * nwno / cols, 1)
    res["host_loop_scaled"] = bool(cols < nwno)
    res["levels_equal_host_loop"] = bool(np.array_equal(levels[:3, :cols], ref))
    print(json.dumps(res))
    return 0 if res["levels_equal_host_loop"] and res["case_equals_dict"] else 1


if __name__ == "__main__":
    sys.exit(main())
