#!/usr/bin/env python
"""get_contribution at 1e5 wavelengths x 90 layers (synthetic.opacity_tables + synthetic.cloud_slab: 2 CIA pairs, 2
molecules, rayleigh, cloud = 6 species) -- run on the GPU box.

    python tools/contribution_time.py [OUT.json]

Reports the end-to-end time of get_contribution (set-up, both kernels, the three device-to-host copies), the time of
one species_opacity() call on the stream timer, the bytes the kernels write and the fraction of 6.3 TB/s; then runs itself
again under ``rocprofv3 --kernel-trace --stats`` (a fresh child process, ``--child``: a few calls and nothing else) and
adds the per-kernel averages of k_opacity_gas<3> (species planes) and k_contribution_columns (sums + tau-pressure)."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NWNO, NLAYER = 100000, 90
HBM_TBS = 6.3


def setup():
    from picaso_amd import justdoit as jdi
    from picaso_amd import optics as px
    from picaso_amd import synthetic as syn
    opa = px.RetrieveOpacities(query_method="linear", **syn.opacity_tables(NWNO))
    nlevel = NLAYER + 1
    plev = np.logspace(-6, 2, nlevel)
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=2500.0)
    case.atmosphere(df={"pressure": plev, "temperature": 150.0 + 1200.0 * ((np.log10(plev) + 6) / 8) ** 2,
                        "H2": np.full(nlevel, 0.84), "He": np.full(nlevel, 0.155), "H2O": np.full(nlevel, 1e-3),
                        "CH4": np.full(nlevel, 5e-4)})
    case.clouds(df=syn.cloud_slab(NLAYER, NWNO))
    case.approx(raman="none")
    return jdi, case, opa


def child():
    jdi, case, opa = setup()
    for _ in range(5):
        jdi.get_contribution(case, opa, at_tau=1.0)


def kernel_stats():
    """Average duration [ms] of the two kernels under rocprofv3 --kernel-trace --stats (None when it is not there)."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None
    out = tempfile.mkdtemp(prefix="contrib_prof_")
    try:
        subprocess.run(["timeout", "-k", "10", "600", exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
                        "-o", "run", "--",
                        sys.executable, os.path.abspath(__file__), "--child"], check=True, stdout=subprocess.DEVNULL)
        res = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for key, tag in (("k_opacity_gas<3>", "species_planes"), ("k_contribution_columns", "columns")):
                        if key in name:
                            res[tag + "_ms"] = float(row["AverageNs"]) * 1e-6
                            res[tag + "_calls"] = int(row["Calls"])
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    from picaso_amd import device
    from picaso_amd import optics as px
    from picaso_amd.spectrum import _setup_atmosphere
    jdi, case, opa = setup()
    ctx = opa.ctx
    out = jdi.get_contribution(case, opa, at_tau=1.0)          # warm-up
    nsp = len(out["taus_per_layer"])
    e2e = []
    for _ in range(5):
        t0 = time.perf_counter()
        jdi.get_contribution(case, opa, at_tau=1.0)
        e2e.append(time.perf_counter() - t0)
    atm = _setup_atmosphere(case.inputs, opa, opa.wno)
    opa.get_opacities(atm)
    keep = px.species_opacity(atm, opa, at_tau=1.0)
    device.sync(ctx)
    kern = []
    for _ in range(5):
        device.timer_start(ctx)
        keep = px.species_opacity(atm, opa, at_tau=1.0)
        kern.append(device.timer_stop(ctx))
    del keep
    written = 8 * nsp * (NLAYER + (NLAYER + 1) + 1) * NWNO
    # the stream timer spans the whole species_opacity() call, host work between the launches included
    res = dict(nwno=NWNO, nlayer=NLAYER, species=list(out["taus_per_layer"]), end_to_end_ms=1e3 * min(e2e),
               call_stream_timer_ms=min(kern), bytes_written=written, d2h_bytes=written)
    stats = kernel_stats()
    if stats:
        res.update(stats)
        if "species_planes_ms" in stats and "columns_ms" in stats:
            res["kernels_ms"] = stats["species_planes_ms"] + stats["columns_ms"]
    t = res.get("kernels_ms", res["call_stream_timer_ms"])
    res["write_rate_TBs"] = written / (t * 1e-3) / 1e12
    res["fraction_of_hbm"] = res["write_rate_TBs"] / HBM_TBS
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main()
