#!/usr/bin/env python
"""What the contribution functions cost at 1e5 wavelengths x 90 layers (resident synthetic opacity tables, the atmosphere
of tools/bench_regrid.py), on an MI355X:

  case_thermal / case_transmission   ``jdi.thermal_contribution(case, opa)`` (R = 100) and
                                     ``jdi.transmission_contribution(case, opa)`` (R = None), host time per call
  k_thermal_cf / k_transit_cf / k_mean_regrid_plane   each kernel alone on resident planes (device timer)
  transit_once / transit_nlayer_plus_1   the only way before: one ``picaso_get_transit_1d_dev`` launch, and the
                                     ``nlayer + 1`` of them the reference's formulation needs, in the same run

Medians over BLOCKS blocks of the mean of CALLS calls, ms.  One JSON line; ``cheaper_than_nlayer_plus_1`` is the only
requirement, ``ratio_to_one_transit`` is recorded."""
import ctypes
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
from picaso_amd import _lib, device, resident    # noqa: E402
from picaso_amd import justdoit as jdi           # noqa: E402
from picaso_amd.atmsetup import _Consts as C     # noqa: E402
from picaso_amd.contribution import _from_case, cf_grid       # noqa: E402
from picaso_amd.device import DeviceArray        # noqa: E402

_ci, _cd, _cl = ctypes.c_int, ctypes.c_double, ctypes.c_long


def median_ms(fn, nblocks, calls, ctx=None):
    """median over blocks of the mean ms per call: host clock, or the device timer around the block when ``ctx``"""
    out = []
    for _ in range(nblocks):
        if ctx is not None:
            device.timer_start(ctx)
            for _ in range(calls):
                fn()
            out.append(device.timer_stop(ctx) / calls)
        else:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            out.append(1e3 * (time.perf_counter() - t0) / calls)
    return round(statistics.median(out), 4)


def main():
    nblocks, calls = int(os.environ.get("BLOCKS", "7")), int(os.environ.get("CALLS", "10"))
    case, opa = world()
    lib, ctx = _lib.load(), opa.ctx
    res = {"nwno": opa.nwno, "nlayer": 90}
    jdi.thermal_contribution(case, opa)
    jdi.transmission_contribution(case, opa)
    res["case_thermal_ms"] = median_ms(lambda: jdi.thermal_contribution(case, opa), nblocks, calls)
    res["case_transmission_ms"] = median_ms(lambda: jdi.transmission_contribution(case, opa), nblocks, calls)
    full, (taugas, taucld, tauray), wno, _, _ = _from_case(case, opa, "1d")
    lay, lev = full["layer"], full["level"]
    nlayer, nwno = len(lay["pressure"]), opa.nwno
    nlevel = nlayer + 1
    d_wno = DeviceArray.from_host(wno, ctx)
    cf_t, cf_x = DeviceArray((nlayer - 1, nwno), ctx), DeviceArray((nlayer, nwno), ctx)
    dtau, depth = DeviceArray((nlayer, nwno), ctx), DeviceArray((nwno,), ctx)
    resident.axpby(ctx, 1.0, taugas, 1.0, tauray, dtau)
    tl, dlnp = _lib.f64(lay["temperature"]), _lib.f64(np.diff(np.log(lay["pressure"])))
    host = [_lib.f64(x) for x in (lev["z"], lev["dz"], lay["mmw"], np.asarray(lev["pressure"]) * C.pconv,
                                  lev["temperature"], lay["column_density"])]
    z, dz, mmw, pl, tlv, cd = (_lib.ptr(x) for x in host)

    def thermal():
        _lib.check(lib.picaso_thermal_cf_dev(ctx, _ci(nlayer), _ci(nwno), _cl(nwno), _lib.ptr(taugas.addr), None,
                                             _lib.ptr(tauray.addr), _lib.ptr(tl), _lib.ptr(d_wno.addr), _lib.ptr(dlnp),
                                             _cd(1.0), _lib.ptr(cf_t.addr)), ctx)

    def transit_cf():
        _lib.check(lib.picaso_transit_cf_dev(ctx, z, dz, _ci(nlevel), _ci(nwno), _cl(nwno), _cd(1.0), mmw, _cd(C.k_b),
                                             _cd(C.amu), pl, tlv, cd, _lib.ptr(dtau.addr), _lib.ptr(cf_x.addr)), ctx)

    def transit():
        _lib.check(lib.picaso_get_transit_1d_dev(ctx, z, dz, _ci(nlevel), _ci(nwno), _cl(nwno), _cd(1.0), mmw, _cd(C.k_b),
                                                 _cd(C.amu), pl, tlv, cd, _lib.ptr(dtau.addr), _lib.ptr(depth.addr)), ctx)

    def transit_all():
        for _ in range(nlayer + 1):
            transit()
    _, plan = cf_grid(opa, 100)
    binned = DeviceArray((nlayer, plan.nbins), ctx)
    d_start = plan.device_start(ctx)

    def regrid():
        _lib.check(lib.picaso_mean_regrid_plane_dev(ctx, _ci(nlayer), _cl(nwno), _cl(nwno), _ci(plan.nbins),
                                                    ctypes.c_void_p(d_start.addr), _lib.ptr(cf_x.addr),
                                                    _lib.ptr(binned.addr)), ctx)
    for name, fn in (("k_thermal_cf_ms", thermal), ("k_transit_cf_ms", transit_cf), ("k_mean_regrid_plane_ms", regrid),
                     ("transit_once_ms", transit), ("transit_nlayer_plus_1_ms", transit_all)):
        fn()
        device.sync(ctx)
        res[name] = median_ms(fn, nblocks, calls, ctx)
    res["ratio_to_one_transit"] = round(res["k_transit_cf_ms"] / res["transit_once_ms"], 2)
    res["cheaper_than_nlayer_plus_1"] = bool(res["k_transit_cf_ms"] < res["transit_nlayer_plus_1_ms"])
    print(json.dumps(res))
    return 0 if res["cheaper_than_nlayer_plus_1"] else 1


if __name__ == "__main__":
    sys.exit(main())
