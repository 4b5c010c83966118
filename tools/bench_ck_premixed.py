#!/usr/bin/env python
"""What the mixture of a premixed correlated-k table costs per P-T point: M = 12 synthetic rows of 2e6 line-by-line cross
sections (``bench_ck_factory.world``'s rows, one seed per gas) with abundances spread over ten decades, binned into 661 bins
at 8 Gauss points.

  (a) fused     ``of.compute_ck_of_sums``: the M rows uploaded one behind the other, summed in HBM
                (``picaso_xsec_axpy_dev``), the sum binned where it lies; only the table comes back
  (b) today     the numpy sum ``s = 0; s += w * d`` on one host core, then ``jdi.compute_ck`` of it (a second upload)
  (c) kernel    the M launches of ``picaso_xsec_axpy_dev`` alone on resident rows (device timer), and the bytes they move
  (d) own grids ``of.weighted_sum`` with every gas on a grid of its own (shifted against the grid of the sum): M
                interpolating launches, M + 1 grid uploads; the sum stays on the device

Per variant: the median over BLOCKS blocks of the mean of CALLS calls (ms per P-T point).  Also whether (a) and (b) give the
same table bit for bit and (d) numpy's bits.  One JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_ck_factory import NBINS, NLBL, blocks        # noqa: E402
from picaso_amd import _lib                             # noqa: E402
from picaso_amd import justdoit as jdi                  # noqa: E402
from picaso_amd import opacity_factory as of            # noqa: E402
from picaso_amd import optics                           # noqa: E402
from picaso_amd.device import DeviceArray, sync, timer_start, timer_stop          # noqa: E402

NGAS = 12


def world(nlbl=NLBL, nbins=NBINS, ngas=NGAS):
    rng = np.random.default_rng(2121)
    og = of.uniform_grid(nlbl, (33333.0 - 33.0) / (nlbl - 1), 33.0)
    rows = []
    for _ in range(ngas):
        row = np.exp(rng.normal(-50.0, 4.0, nlbl)) + 1e-27
        row[rng.uniform(size=nlbl) < 0.01] = 0.0
        rows.append(row)
    weights = 10.0 ** rng.uniform(-12.0, -2.0, ngas)
    weights[0] = 0.84                                   # H2
    edges = np.geomspace(og[0] * 0.999, og[-1] * 1.001, nbins + 1)
    return rows, weights, og, edges[:-1], edges[1:], optics.g_w_2gauss(4, 0.95)[0]


def numpy_sum(rows, weights):
    s = 0
    for w, d in zip(weights, rows):
        s += w * d
    return s


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    nblocks, calls = int(os.environ.get("BLOCKS", "5")), int(os.environ.get("CALLS", "3"))
    rows, weights, og, low, high, g = world(int(os.environ.get("NLBL", NLBL)), int(os.environ.get("NBINS", NBINS)),
                                            int(os.environ.get("NGAS", NGAS)))
    nlbl, ngas = int(og.size), len(rows)
    res = {"n_lbl": nlbl, "ngas": ngas, "nbins": int(low.size), "ngauss": int(g.size)}
    point = [(rows, weights)]

    def fused():
        return of.compute_ck_of_sums(point, [og], low, high, g)

    def today():
        return jdi.compute_ck(numpy_sum(rows, weights), og, low, high, g)

    res["fused_equals_today_bitwise"] = bool(np.array_equal(bits(fused()), bits(today())))      # also the warm-up
    fused()
    res["fused_ms"] = blocks(fused, nblocks, calls)
    res["today_ms"] = blocks(today, nblocks, calls)
    res["today_host_sum_ms"] = blocks(lambda: numpy_sum(rows, weights), nblocks, calls)
    s = numpy_sum(rows, weights)
    res["today_compute_ck_ms"] = blocks(lambda: jdi.compute_ck(s, og, low, high, g), nblocks, calls)

    # (c) the kernel alone
    ctx, lib = _lib.context(), _lib.load()
    d_rows = [DeviceArray.from_host(r, ctx) for r in rows]
    d_acc = DeviceArray((nlbl,), ctx)

    def launches():
        for m in range(ngas):
            _lib.check(lib.picaso_xsec_axpy_dev(ctx, nlbl, d_acc.addr, int(m == 0), float(weights[m]), d_rows[m].addr, nlbl,
                                                None, None, 0.0, 0.0), ctx)

    launches()
    sync(ctx)
    res["kernel_sum_equals_numpy_bitwise"] = bool(np.array_equal(bits(d_acc.to_host()), bits(s)))
    times = []
    for _ in range(nblocks * calls):
        timer_start(ctx)
        launches()
        times.append(timer_stop(ctx))
    res["kernel_ms"] = round(statistics.median(times), 4)
    moved = 8.0 * nlbl * (3 * ngas - 1)                 # the first launch does not read the sum
    res["kernel_tb_per_s"] = round(moved / (res["kernel_ms"] * 1e-3) / 1e12, 3)
    for d in d_rows + [d_acc]:
        d.free()

    # (d) every gas on its own grid
    step = float(og[1] - og[0])
    grids = [of.uniform_grid(nlbl, step * (1.0 + 1e-3 * (m % 3 - 1)), 33.0 + 0.37 * step * m) for m in range(ngas)]
    t0 = time.perf_counter()
    want = numpy_sum([np.interp(og, gm, r) for gm, r in zip(grids, rows)], weights)
    res["own_grids_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)

    def own_grids():
        of.weighted_sum(rows, weights, grids=grids, out_grid=og, out="device").free()

    res["own_grids_equals_numpy_bitwise"] = bool(np.array_equal(
        bits(of.weighted_sum(rows, weights, grids=grids, out_grid=og)), bits(want)))
    res["own_grids_ms"] = blocks(own_grids, max(1, nblocks // 2), max(1, calls // 2))
    res["fused_below_today"] = bool(res["fused_ms"] < res["today_ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
