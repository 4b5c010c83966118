#!/usr/bin/env python
"""What binning to an instrument grid costs per call of the headline synthetic workload (1e5 wavelengths x 90 layers x 5
disk angles, ``spectrum('reflected+thermal')`` with a star, resident synthetic opacity tables), for R = 100 and R = 1000:

  (a) host      ``spectrum()`` followed by ``jdi.mean_regrid`` of each of the five spectral arrays (the way before regrid=)
  (b) regrid    ``spectrum(regrid={'R': R})``: binned on the device, nbins doubles per array copied back
  (c) plain     ``spectrum()`` alone

and the same three with ``spectrum_async`` pipelined (call i + 1 is enqueued before call i is read).  Per variant: the
median over BLOCKS blocks of the mean of CALLS calls (ms per call).  One JSON line.  REGRID_PROFILE=1: 200 calls of (b)
at R = 100 and nothing else, for ``rocprofv3 --kernel-trace --stats -- python tools/bench_regrid.py`` (the kernel's own
time is the k_mean_regrid row)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib                      # noqa: E402
from picaso_amd import justdoit as jdi           # noqa: E402
from picaso_amd import optics as px              # noqa: E402
from picaso_amd import synthetic as syn          # noqa: E402

KEYS = ("albedo", "fpfs_reflected", "thermal", "fpfs_thermal", "fpfs_total")


def world(nwno=100000, nlevel=91):
    wno = np.linspace(2000.0, 33333.0, nwno)
    tabs = syn.opacity_tables(nwno, wno=wno)
    opa = px.RetrieveOpacities(tabs["wno"], tabs["pt_pairs"], tabs["molecular"], tabs["continuum"], tabs["cia_temps"],
                               rayleigh_opa=tabs["rayleigh_opa"], query_method="linear", ctx=_lib.context(0))
    plev = np.logspace(-6, 2, nlevel)
    prof = {"pressure": plev, "temperature": 150.0 + 1200.0 * ((np.log10(plev) + 6) / 8) ** 2, "H2": np.full(nlevel, 0.84),
            "He": np.full(nlevel, 0.155), "H2O": np.full(nlevel, 1e-3), "CH4": np.full(nlevel, 5e-4)}
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(radius=7.1e9, mass=1.9e30)
    case.atmosphere(df=prof)
    case.approx(raman="none")
    case.star(relative_flux=1.0 + 0.2 * np.cos(wno / 900.0), radius=6.9e10, semi_major=7.5e12)
    return case, opa


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
    case, opa = world(int(os.environ.get("NWNO", "100000")))
    if os.environ.get("REGRID_PROFILE"):
        for _ in range(200):
            case.spectrum(opa, calculation=calc, regrid={"R": 100})
        return
    res = {"nwno": opa.nwno, "blocks": nblocks, "calls_per_block": calls}

    def host_bin(out, R):
        return [jdi.mean_regrid(out["wavenumber"], out[k], R=R)[1] for k in KEYS]

    def pipelined(start, finish):
        def run(n):
            prev = start()
            for _ in range(n - 1):
                nxt = start()
                finish(prev.result())
                prev = nxt
            finish(prev.result())
        return run

    for R in (100, 1000):
        spec = {"R": R}
        plan = jdi.regrid_plan(opa, R=R)
        plain = case.spectrum(opa, calculation=calc)
        binned = case.spectrum(opa, calculation=calc, regrid=spec)
        same = all(np.array_equal(binned[k], m, equal_nan=True) for k, m in zip(KEYS, host_bin(plain, R)))
        variants = {
            "host": lambda n: [host_bin(case.spectrum(opa, calculation=calc), R) for _ in range(n)],
            "regrid": lambda n: [case.spectrum(opa, calculation=calc, regrid=spec) for _ in range(n)],
            "plain": lambda n: [case.spectrum(opa, calculation=calc) for _ in range(n)],
            "async_host": pipelined(lambda: case.spectrum_async(opa, calculation=calc), lambda o: host_bin(o, R)),
            "async_regrid": pipelined(lambda: case.spectrum_async(opa, calculation=calc, regrid=spec), lambda o: None),
            "async_plain": pipelined(lambda: case.spectrum_async(opa, calculation=calc), lambda o: None),
        }
        r = {"nbins": plan.nbins, "bit_identical_to_host": bool(same)}
        for name, fn in variants.items():
            fn(5)                                   # warm-up: block tables, pinned blocks, plan upload
        for name, fn in variants.items():
            r[name + "_ms"] = blocks(fn, nblocks, calls)
        r["regrid_minus_plain_ms"] = round(r["regrid_ms"] - r["plain_ms"], 4)
        res["R%d" % R] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
