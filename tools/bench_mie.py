#!/usr/bin/env python
"""What a Mie table and a batch of Mie cloud tables cost on the GPU against the host routes (GPU only; one JSON line).

  mieff     ``mie.compute_mieff`` at 196 wavelengths (0.3 - 30 micron) x 60 radii (1e-7 - 5e-2 cm) x 6 sub-radii = 70 560
            Mie series of up to ~2e4 terms, as a whole (sort, uploads, the launches of ``picaso_mie_q_dev`` in chunks, the
            copies back, the mean), against ``mie_efficiencies_numpy`` timed on a SUBSET -- every 64th series of the list
            sorted by length, so that the subset has the whole list's mix of lengths -- and scaled to the whole list by the
            ratio of the summed series lengths (``numpy_scaled_s``: an estimate, named as one).  The largest difference
            between the two on the subset is reported.
  clouds    ``mie.cloud_tables_batch`` at S = 1000 samples of two decks (a Brewster slab and a flex_fsed deck, parameters
            drawn per sample) on 90 layers x 196 wavelengths as a whole and its host half alone (``records_host``), against
            the host functions per sample (``cloud_brewster_mie``, ``cloud_flex_fsed``, ``cloud_averaging``) timed on the
            first HOST_SAMPLES samples; the rows of those samples are compared bit for bit.

Per figure the median of REPS repetitions with the smallest and the largest beside it."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib, mie                     # noqa: E402
from picaso_amd import justdoit as jdi              # noqa: E402
from picaso_amd import parameterizations as pz      # noqa: E402

REPS = int(os.environ.get("MIE_BENCH_REPS", "5"))
S = int(os.environ.get("MIE_BENCH_SAMPLES", "1000"))
HOST_SAMPLES = int(os.environ.get("MIE_BENCH_HOST_SAMPLES", "20"))
NWAVE, NRADII, NSUB, NLEVEL = 196, 60, 6, 91


def stats_ms(fn, reps=REPS, per=1):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3 / per)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def main():
    _lib.context()
    rng = np.random.default_rng(6)
    wave = np.geomspace(0.3, 30.0, NWAVE)
    nn = 1.5 + 0.2 * np.sin(np.log(wave) * 2.0)
    kk = 10 ** rng.uniform(-6, -0.5, NWAVE)
    radius = np.geomspace(1e-7, 5e-2, NRADII)
    res = {"nwave": NWAVE, "nradii": NRADII, "nsub": NSUB, "series": NWAVE * NRADII * NSUB, "reps": REPS}

    # (a) the table
    sub = mie.sub_radii(radius, None, NSUB)
    x = (2 * mie.PI * sub[None, :, :] / (wave * 1e-4)[:, None, None]).reshape(-1)
    m = np.repeat(nn + 1j * kk, NRADII * NSUB)
    _, nstop, nmx = mie._orders(x, m)
    res["terms_total"], res["terms_longest"] = int(nmx.sum()), int(nmx.max())
    launches = mie.MIE_LAUNCHES
    table = mie.compute_mieff(wave, nn, kk, radius, nsub=NSUB)
    res["chunks"] = mie.MIE_LAUNCHES - launches
    res["compute_mieff"] = stats_ms(lambda: mie.compute_mieff(wave, nn, kk, radius, nsub=NSUB))
    pick = np.argsort(-nmx, kind="stable")[::64]
    t0 = time.perf_counter()
    host = mie.mie_efficiencies_numpy(x[pick], m[pick])
    t_host = time.perf_counter() - t0
    dev = mie.mie_efficiencies(x[pick], m[pick])
    res["numpy_subset"] = {"series": int(pick.size), "terms": int(nmx[pick].sum()), "seconds": t_host}
    res["numpy_scaled_s"] = t_host * res["terms_total"] / res["numpy_subset"]["terms"]
    res["device_vs_numpy_subset"] = {"qext_rel": float(np.max(np.abs(dev[0] - host[0]) / host[0])),
                                     "qsca_rel": float(np.max(np.abs(dev[1] - host[1]) / host[1])),
                                     "g_abs": float(np.max(np.abs(dev[2] - host[2]) / host[1]))}

    # (b) the batch of cloud tables
    plev = np.logspace(-6, 2, NLEVEL)
    case = jdi.inputs()
    case.add_pt(P=plev)
    param = pz.Parameterize()
    param.add_class(case)
    nlayer = NLEVEL - 1
    samples = [[dict(kind="brewster_mie", table=table, distribution="lognorm", decay_type="slab",
                     lognorm_kwargs=dict(sigma=rng.uniform(0.2, 0.8), lograd=rng.uniform(-5.0, -3.0)),
                     slab_kwargs=dict(ptop=rng.uniform(-4.0, -2.0), dp=rng.uniform(0.5, 1.5), reference_tau=rng.uniform(0.1, 2.0))),
                dict(kind="flex_fsed", table=table, distribution="hansen", base_pressure=10 ** rng.uniform(-1.0, 1.0),
                     ndz=10 ** rng.uniform(4.0, 8.0), fsed=rng.uniform(0.3, 3.0),
                     hansen_kwargs=dict(b=rng.uniform(0.05, 0.3), lograd=rng.uniform(-4.5, -3.0)))]
               for _ in range(S)]
    res["clouds"] = {"samples": S, "decks": 2, "nlayer": nlayer, "table_KB_per_sample": 3 * nlayer * NWAVE * 8 / 1e3}
    res["batch"] = stats_ms(lambda: mie.cloud_tables_batch(param, samples))
    res["batch_per_sample"] = {k: v / S for k, v in res["batch"].items()}
    res["records_host"] = stats_ms(lambda: mie._batch_records(param, samples))

    def host_build(sample):
        kws = [{k: v for k, v in d.items() if k != "kind"} for d in sample]
        return pz.cloud_averaging([mie.cloud_brewster_mie(param, **kws[0]), mie.cloud_flex_fsed(param, **kws[1])])
    res["host_per_sample"] = stats_ms(lambda: [host_build(s) for s in samples[:HOST_SAMPLES]], per=HOST_SAMPLES)
    tabs = mie.cloud_tables_batch(param, samples)
    same = True
    for s in range(HOST_SAMPLES):
        df = host_build(samples[s])
        want = np.array([df[k].values for k in ("opd", "w0", "g0")]).reshape(3 * nlayer, NWAVE)
        same = same and bool(np.array_equal(tabs[s].d_stack.to_host().view(np.uint64), want.view(np.uint64)))
    res["rows_equal_bit_for_bit"] = same
    print(json.dumps(res))


if __name__ == "__main__":
    main()
