#!/usr/bin/env python
"""What making a correlated-k table costs per P-T point: ONE synthetic row of 2e6 line-by-line cross sections (log-normal
lines on a continuum, 1 % zeros) binned into the 661 bins of a constant-R grid at 8 Gauss points (``g_w_2gauss(4, 0.95)``):

  (a) device   ``jdi.compute_ck`` on the row (upload, both kernels, the table back), and the same with every segment sent
               through the HBM selection path (``_lds_cap=1``)
  (b) host     the numpy restatement of the reference's bin loop (opacity_factory.py:1927-1955): mask, clamp,
               ``np.sort(np.log(...))``, ``np.interp`` per bin

Per variant: the median over BLOCKS blocks of the mean of CALLS calls (ms per row).  Also: the segment lengths and the worst
``|device - host| / bound`` (``bound = 8 * 2^-53 * max|ln|`` of the two order statistics).  One JSON line.  HOST_ONLY=1: (b)
alone, no GPU needed.  CK_PROFILE=1: 50 calls of (a) and nothing else, for ``rocprofv3 --kernel-trace --stats -- python
tools/bench_ck_factory.py`` (the kernels' own times are the k_ck_sort_lds and k_ck_select_hbm rows)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from picaso_amd import justdoit as jdi                  # noqa: E402
from picaso_amd import opacity_factory as of            # noqa: E402
from picaso_amd import optics                           # noqa: E402
from test_ck_factory import restate_ck as restate       # noqa: E402  (the numpy oracle of the tests)

NLBL, NBINS = 2_000_000, 661


def world(nlbl=NLBL, nbins=NBINS):
    """``(row, og, low, high, g)``: a uniform grid from 33 to 33 333 cm^-1 (0.3-300 um) and ``nbins`` constant-R bins on it."""
    rng = np.random.default_rng(1460)
    og = of.uniform_grid(nlbl, (33333.0 - 33.0) / (nlbl - 1), 33.0)
    row = np.exp(rng.normal(-50.0, 4.0, nlbl)) + 1e-27
    row[rng.uniform(size=nlbl) < 0.01] = 0.0
    edges = np.geomspace(og[0] * 0.999, og[-1] * 1.001, nbins + 1)
    return row, og, edges[:-1], edges[1:], optics.g_w_2gauss(4, 0.95)[0]


def blocks(fn, nblocks, calls):
    """median over ``nblocks`` of the mean ms per call of ``calls`` calls"""
    out = []
    for _ in range(nblocks):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return round(statistics.median(out), 4)


def main():
    nblocks, calls = int(os.environ.get("BLOCKS", "5")), int(os.environ.get("CALLS", "4"))
    host_blocks, host_calls = int(os.environ.get("HOST_BLOCKS", "3")), int(os.environ.get("HOST_CALLS", "1"))
    row, og, low, high, g = world(int(os.environ.get("NLBL", NLBL)), int(os.environ.get("NBINS", NBINS)))
    n = of.ck_segments(og, low, high)[1]
    res = {"n_lbl": int(row.size), "nbins": int(low.size), "ngauss": int(g.size), "segment_min": int(n.min()),
           "segment_median": int(np.median(n)), "segment_max": int(n.max()), "segments_above_lds_cap": int((n > 16384).sum())}
    if os.environ.get("CK_PROFILE"):
        for _ in range(50):
            jdi.compute_ck(row, og, low, high, g)
        return
    if not os.environ.get("HOST_ONLY"):
        k, stats = jdi.compute_ck(row, og, low, high, g, _return_stats=True)
        ref = restate(row, og, low, high, g)
        bound = 8.0 * 2.0 ** -53 * np.max(np.abs(np.log(stats[0])), axis=2)
        ok = n >= 2
        res["worst_error_over_bound"] = round(float(np.max(np.abs(k[0] - ref)[ok] / bound[ok])), 4)
        res["empty_bins_exact"] = bool(np.all(k[0][~ok] == -200.0))
        for _ in range(2):                                                  # warm-up: pinned blocks, device buffers
            jdi.compute_ck(row, og, low, high, g)
        res["device_ms"] = blocks(lambda: jdi.compute_ck(row, og, low, high, g), nblocks, calls)
        res["device_hbm_path_ms"] = blocks(lambda: jdi.compute_ck(row, og, low, high, g, _lds_cap=1), nblocks, calls)
        res["segments_ms"] = blocks(lambda: of.ck_segments(og, low, high), nblocks, calls)
    res["host_ms"] = blocks(lambda: restate(row, og, low, high, g), host_blocks, host_calls)
    if "device_ms" in res:
        res["device_below_host"] = bool(res["device_ms"] < res["host_ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
