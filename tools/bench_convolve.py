#!/usr/bin/env python
"""What convolving with an instrument's line-spread function costs per call of the headline synthetic workload (1e5
wavelengths x 90 layers x 5 disk angles, ``spectrum('reflected+thermal')`` with a star, resident synthetic opacity
tables), for 400 data points over 0.32-4.9 um at R = 100 and at R rising from 30 to 300 along the spectrum:

  (a) plain     ``spectrum()`` alone
  (b) host      ``spectrum()`` followed by ``jdi.conv_non_uniform_R`` of each of the five spectral arrays (the way before
                convolve=; 400 x 1e5 ``exp`` per array: HOST_CALLS calls per block, 1 by default)
  (c) convolve  ``spectrum(convolve=plan)``: convolved on the device, 400 doubles per array copied back -- alone, and
                pipelined through ``spectrum_async`` (call i + 1 is enqueued before call i is read)

Per variant: the median over BLOCKS blocks of the mean of CALLS calls (ms per call).  Also per case: the window sizes and
the worst ``|device - host| / bound`` over the five arrays (``bound = (2 counts + 10) 2^-53 conv(|array|)``).  One JSON
line.  CONVOLVE_PROFILE=1: 200 calls of (c) at R = 100 and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/bench_convolve.py`` (the kernel's own time is the k_lsf_convolve row)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from picaso_amd import justdoit as jdi           # noqa: E402
from bench_regrid import world                   # noqa: E402

KEYS = ("albedo", "fpfs_reflected", "thermal", "fpfs_thermal", "fpfs_total")
NOBS = 400


def blocks(fn, nblocks, calls):
    """median over ``nblocks`` of the mean ms per call of ``calls`` calls"""
    out = []
    for _ in range(nblocks):
        t0 = time.perf_counter()
        fn(calls)
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return round(statistics.median(out), 4)


def main():
    calc = "reflected+thermal"
    nblocks, calls = int(os.environ.get("BLOCKS", "9")), int(os.environ.get("CALLS", "20"))
    host_blocks, host_calls = int(os.environ.get("HOST_BLOCKS", "3")), int(os.environ.get("HOST_CALLS", "1"))
    case, opa = world(int(os.environ.get("NWNO", "100000")))
    wl = np.linspace(0.32, 4.9, NOBS)
    cases = {"R100": np.full(NOBS, 100.0), "R30to300": np.linspace(30.0, 300.0, NOBS)}
    if os.environ.get("CONVOLVE_PROFILE"):
        plan = jdi.convolve_plan(opa, wl, cases["R100"])
        for _ in range(200):
            case.spectrum(opa, calculation=calc, convolve=plan)
        return
    res = {"nwno": opa.nwno, "nobs": NOBS, "blocks": nblocks, "calls_per_block": calls, "host_blocks": host_blocks,
           "host_calls_per_block": host_calls}

    def pipelined(start):
        def run(n):
            prev = start()
            for _ in range(n - 1):
                nxt = start()
                prev.result()
                prev = nxt
            prev.result()
        return run

    for name, R in cases.items():
        plan = jdi.convolve_plan(opa, wl, R)

        def host_conv(out):
            model_wl = 1e4 / out["wavenumber"]
            return [jdi.conv_non_uniform_R(out[k], model_wl, R, wl) for k in KEYS]

        plain = case.spectrum(opa, calculation=calc)
        conv = case.spectrum(opa, calculation=calc, convolve=plan)
        model_wl = 1e4 / plain["wavenumber"]
        worst = 0.0
        for k, h in zip(KEYS, host_conv(plain)):
            lim = (2.0 * plan.counts + 10.0) * 2.0 ** -53 * jdi.conv_non_uniform_R(np.abs(plain[k]), model_wl, R, wl)
            worst = max(worst, float(np.max(np.abs(conv[k] - h) / lim)))
        r = {"counts_min": int(plan.counts.min()), "counts_median": int(np.median(plan.counts)),
             "counts_max": int(plan.counts.max()), "columns_in_all_windows": int(plan.counts.sum()),
             "worst_error_over_bound": round(worst, 4)}
        variants = {
            "plain": lambda n: [case.spectrum(opa, calculation=calc) for _ in range(n)],
            "convolve": lambda n: [case.spectrum(opa, calculation=calc, convolve=plan) for _ in range(n)],
            "async_plain": pipelined(lambda: case.spectrum_async(opa, calculation=calc)),
            "async_convolve": pipelined(lambda: case.spectrum_async(opa, calculation=calc, convolve=plan)),
        }
        for fn in variants.values():
            fn(5)                                   # warm-up: block tables, pinned blocks, plan upload
        for key, fn in variants.items():
            r[key + "_ms"] = blocks(fn, nblocks, calls)
        r["host_ms"] = blocks(lambda n: [host_conv(case.spectrum(opa, calculation=calc)) for _ in range(n)],
                              host_blocks, host_calls)
        r["convolve_minus_plain_ms"] = round(r["convolve_ms"] - r["plain_ms"], 4)
        r["convolve_below_host"] = bool(r["convolve_ms"] < r["host_ms"] and r["async_convolve_ms"] < r["host_ms"])
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
