#!/usr/bin/env python
"""What a cloudy phase curve costs through ``inputs.clouds_4d`` against the host route it replaces (GPU only; one JSON line).

Shape: one native GCM cloud map, 128 x 64 columns x 52 layers x 196 wavenumbers (3 x 668 MB), 10 x 10 facets, 8 phases,
thermal emission, 12 500 opacity wavelengths x 53 levels of synthetic resident opacity tables.  Measured in one run:

  host_per_phase   the parent's way, per phase: ``_regrid_lonlat`` of opd / w0 / g0 on the rotated map, sorted and transposed
                   as ``clouds_3d`` stores them (``regrid``), then ``optics._facet_major_cloud_tables``: re-stack, fingerprint
                   and upload (``stack_upload``);
  map_upload       ``GcmCloudMap.resident`` of a map not yet in HBM: the content digest and the three uploads, once;
  map_hit          the same call again: the digest alone;
  facet_tables     ``gcm.facet_tables`` for all phases: index tables on the host, one launch, one wait (wall clock), and the
                   device timer around it;
  curve            the whole cloudy ``phase_curve`` both ways: ``clouds_4d(map)`` (map resident) + ``phase_curve(opa)``, and
                   host dictionaries for every phase + ``phase_curve(opa, clouds_by_phase=...)``.

Per figure the median of REPS repetitions with the smallest and the largest beside it."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib, device, gcm            # noqa: E402
from picaso_amd import justdoit as jdi              # noqa: E402
from picaso_amd import optics as px                 # noqa: E402

REPS = int(os.environ.get("CLOUDS4D_BENCH_REPS", "5"))
NLON, NLAT, NLEVEL, NIN = (int(x) for x in os.environ.get("CLOUDS4D_BENCH_SHAPE", "128,64,53,196").split(","))
NG = NT = 10
NPHASE = 8
NWNO = int(os.environ.get("CLOUDS4D_BENCH_NWNO", "12500"))


def stats_ms(fn, reps=REPS):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def opacities(ctx):
    wno = np.linspace(2000.0, 33333.0, NWNO)
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


def host_tables(cloud, lon_f, lat_f, phase, shift):
    """One phase the host way: rotate, ``_regrid_lonlat``, sort and transpose as ``clouds_3d`` does."""
    lon_rot = (cloud["lon"] + phase * 180 / np.pi + shift + 180.0) % 360.0 - 180.0
    v = jdi._regrid_lonlat({"lon": lon_rot, "lat": cloud["lat"]}, {k: cloud[k] for k in ("opd", "w0", "g0")}, lon_f, lat_f)
    order, worder = np.argsort(cloud["pressure"]), np.argsort(cloud["wno"])
    out = {k: np.ascontiguousarray(np.transpose(v[k][:, :, order][:, :, :, worder], (2, 3, 0, 1))) for k in ("opd", "w0", "g0")}
    out["wavenumber"] = cloud["wno"][worder]
    return out


def main():
    ctx = _lib.context()
    opa = opacities(ctx)
    rng = np.random.default_rng(3)
    lon, lat = np.linspace(-180.0, 180.0, NLON, endpoint=False), np.linspace(-90.0, 90.0, NLAT)
    plev = np.logspace(-6, 2, NLEVEL)
    tlev = 150.0 + 1200.0 * ((np.log10(plev) + 6) / 8) ** 2
    day = 1.0 + 0.1 * np.cos(np.radians(lon))[:, None, None] * np.cos(np.radians(lat))[None, :, None]
    gcm_map = {"lon": lon, "lat": lat, "pressure": plev, "temperature": day * tlev[None, None, :]}
    for m, x in (("H2", 0.84), ("He", 0.155), ("H2O", 1e-3), ("CH4", 5e-4), ("CO", 1e-4), ("NH3", 1e-5)):
        gcm_map[m] = np.full((NLON, NLAT, NLEVEL), x)
    shape = (NLON, NLAT, NLEVEL - 1, NIN)
    cloud = {"lon": lon, "lat": lat, "pressure": np.sqrt(plev[1:] * plev[:-1]), "wno": np.linspace(opa.wno[0], opa.wno[-1], NIN),
             "opd": 0.3 * rng.random(shape), "w0": 0.5 + 0.45 * rng.random(shape), "g0": 0.7 * rng.random(shape)}
    cloud["opd"][:, :, :NLEVEL // 2] = 0.0
    phases = [float(p) for p in np.linspace(0.0, 2 * np.pi, NPHASE, endpoint=False)]

    def case():
        c = jdi.inputs()
        c.gravity(gravity=2500.0)
        c.approx(raman="none")
        c.phase_curve_geometry("thermal", phases, num_gangle=NG, num_tangle=NT)
        c.atmosphere_4d(gcm_map, verbose=False)
        return c
    base = case()
    geom, shift = base.inputs["disco"], base.inputs["shift"]
    lon_f = [geom[ph]["longitude"] * 180 / np.pi for ph in phases]
    lat_f = [geom[ph]["latitude"] * 180 / np.pi for ph in phases]
    res = {"map": [NLON, NLAT, NLEVEL - 1, NIN], "map_MB": 3 * np.prod(shape) * 8 / 1e6, "facets": [NG, NT], "phases": NPHASE,
           "nwno": NWNO, "reps": REPS, "tables_MB_per_phase": 3 * NG * NT * (NLEVEL - 1) * NIN * 8 / 1e6}

    # (a) the parent's way, per phase (phase 1: rotated off the map's own columns)
    res["host_per_phase_regrid"] = stats_ms(lambda: host_tables(cloud, lon_f[1], lat_f[1], phases[1], shift[1]))

    def stack_upload():
        px._facet_major_cloud_tables(fresh.pop(), NLEVEL - 1, NG * NT, ctx)
        device.sync(ctx)
    host_tables_1 = host_tables(cloud, lon_f[1], lat_f[1], phases[1], shift[1])
    # new arrays every time, made outside the clock: the memo is kept by identity and content
    fresh = [{k: v.copy() for k, v in host_tables_1.items()} for _ in range(REPS + 1)]
    res["host_per_phase_stack_upload"] = stats_ms(stack_upload)

    # (b) the map, once
    coords, variables = jdi._dataset_like(cloud, extra_coords=("wno",))

    def upload():
        gcm.clear_map_cache()
        gcm.GcmCloudMap.resident(coords, variables, ctx)
        device.sync(ctx)
    res["map_upload"] = stats_ms(upload, reps=max(2, REPS // 2))
    cmap = gcm.GcmCloudMap.resident(coords, variables, ctx)
    res["map_hit"] = stats_ms(lambda: gcm.GcmCloudMap.resident(coords, variables, ctx))

    # (c) all phases in one launch
    rot = [(ph * 180 / np.pi, shift[i]) for i, ph in enumerate(phases)]
    res["facet_tables"] = stats_ms(lambda: gcm.facet_tables(cmap, lon_f, lat_f, rot))
    times = []
    for _ in range(REPS):
        device.timer_start(ctx)
        gcm.facet_tables(cmap, lon_f, lat_f, rot)
        times.append(device.timer_stop(ctx))
    res["facet_tables_device_ms"] = statistics.median(times)
    res["facet_tables_traffic_GBps"] = 5 * NPHASE * res["tables_MB_per_phase"] / res["facet_tables_device_ms"]

    # (d) the whole cloudy curve, both ways
    def new_way():
        c = case_new
        c.clouds_4d(cloud, plot=False, verbose=False, calculation="thermal")
        return c.phase_curve(opa)

    def old_way():
        host = [host_tables(cloud, lon_f[i], lat_f[i], ph, shift[i]) for i, ph in enumerate(phases)]
        return case_old.phase_curve(opa, clouds_by_phase=host)
    case_new, case_old = case(), case()
    a, b = new_way(), old_way()
    res["curves_equal"] = bool(all(np.array_equal(a[ph]["thermal"], b[ph]["thermal"]) for ph in phases))
    res["curve_clouds_4d"] = stats_ms(new_way)
    res["curve_host_clouds_by_phase"] = stats_ms(old_way)

    def gpu_only():
        return case_new.phase_curve(opa)
    res["curve_phase_curve_alone_tables_resident"] = stats_ms(gpu_only)
    res["speedup_curve"] = res["curve_host_clouds_by_phase"]["median_ms"] / res["curve_clouds_4d"]["median_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
