#!/usr/bin/env python
"""What a parametrized grey cloud costs per sample of a retrieval, made in HBM by ``Parameterize.cloud_tables_batch`` against
the host route it replaces (GPU only; one JSON line).

Shape: 1 000 samples of a two-deck grey cloud (a slab above a deck, parameters drawn per sample) on 90 layers x 196
wavenumbers, spectra on 12 500 opacity wavelengths x 91 levels of synthetic resident opacity tables.  Measured in one run:

  launch            ``picaso_param_cloud_tables_dev`` for all samples by the device timer, and the traffic that is
                    (24 bytes written per element);
  batch             ``cloud_tables_batch`` as a whole: the layer vectors on the host (``records_host`` alone), two uploads,
                    the launch, one wait;
  host_per_sample   the reference-style host build of one sample: two ``cloud_brewster_grey`` DataFrames and
                    ``cloud_averaging``;
  digest_upload     what the spectrum then does with a host table of that size: the (3 * nlayer, nin) stack, its digest and
                    the upload (``onecall._cloud_inputs`` + ``_fill_block_opacity``);
  spectra           ``spectrum_batch`` over NSPEC of the samples fed the tables made in HBM, and over the same cases fed
                    host dictionaries of the same values (made outside the clock), per spectrum.

Per figure the median of REPS repetitions with the smallest and the largest beside it."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from picaso_amd import _lib, device                  # noqa: E402
from picaso_amd import justdoit as jdi              # noqa: E402
from picaso_amd import optics as px                 # noqa: E402
from picaso_amd import parameterizations as pz      # noqa: E402
from bench_clouds4d import opacities                # noqa: E402

REPS = int(os.environ.get("PARAM_CLOUDS_BENCH_REPS", "5"))
S = int(os.environ.get("PARAM_CLOUDS_BENCH_SAMPLES", "1000"))
NSPEC = int(os.environ.get("PARAM_CLOUDS_BENCH_SPECTRA", "64"))
NLEVEL, NIN = 91, 196


def stats_ms(fn, reps=REPS, per=1):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3 / per)
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def cloud_grid(wno):
    """A $picaso_refdata whose wave_EGP.dat is a 196-point grid inside the opacity grid."""
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "opacities"))
    grid = np.round(np.geomspace(wno[0] * 1.01, wno[-1] * 0.99, NIN), 2)
    with open(os.path.join(d, "opacities", "wave_EGP.dat"), "w") as fh:
        fh.write("   i   wavenumber\n")
        for i, w in enumerate(grid[::-1]):
            fh.write("%4d %.2f\n" % (i + 1, w))
    os.environ["picaso_refdata"] = d


def main():
    ctx = _lib.context()
    opa = opacities(ctx)
    cloud_grid(opa.wno)
    grid = jdi.get_cld_input_grid()
    rng = np.random.default_rng(4)
    plev = np.logspace(-6, 2, NLEVEL)
    tlev = 150.0 + 1200.0 * ((np.log10(plev) + 6) / 8) ** 2
    prof = {"pressure": plev, "temperature": tlev}
    prof.update({m: np.full(NLEVEL, x) for m, x in (("H2", 0.84), ("He", 0.155), ("H2O", 1e-3), ("CH4", 5e-4))})

    def case(clouds=None):
        c = jdi.inputs()
        c.phase_angle(0)
        c.gravity(gravity=2500.0)
        c.atmosphere(df=prof)
        c.approx(raman="none")
        if clouds is not None:
            c.clouds(df=clouds, wavenumber=grid)
        return c
    param = pz.Parameterize()
    param.add_class(case())
    samples = [[dict(kind="brewster_grey", decay_type="slab", alpha=rng.uniform(0.0, 3.0), ssa=rng.uniform(0.5, 1.0),
                     reference_wave=1.0, slab_kwargs=dict(ptop=rng.uniform(-4.0, -2.0), dp=rng.uniform(0.5, 1.5),
                                                          reference_tau=rng.uniform(0.1, 2.0))),
                dict(kind="brewster_grey", decay_type="deck", alpha=rng.uniform(-1.0, 1.0), ssa=rng.uniform(0.2, 0.9),
                     reference_wave=1.0, deck_kwargs=dict(ptop=rng.uniform(-1.0, 1.0), dp=rng.uniform(0.1, 1.0)))]
               for _ in range(S)]
    nlayer = NLEVEL - 1
    res = {"samples": S, "decks": 2, "nlayer": nlayer, "nin": NIN, "nwno": int(opa.nwno), "reps": REPS,
           "table_KB_per_sample": 3 * nlayer * NIN * 8 / 1e3}

    # (a) the launch alone and the batch as a whole
    res["batch"] = stats_ms(lambda: param.cloud_tables_batch(samples))
    res["batch_per_sample"] = {k: v / S for k, v in res["batch"].items()}
    res["records_host"] = stats_ms(lambda: param._batch_records(samples))
    layers, params, average, _ = param._batch_records(samples)
    grids = param._resident_grids(ctx)
    d_layers, d_params = device.DeviceArray.from_host(layers, ctx), device.DeviceArray.from_host(params, ctx)
    out = device.DeviceArray((S, 3 * nlayer, NIN), ctx)
    times = []
    for _ in range(REPS + 1):
        device.timer_start(ctx)
        _lib.check(_lib.load().picaso_param_cloud_tables_dev(ctx, S, 2, nlayer, NIN, average, d_layers.addr, d_params.addr,
                                                             grids["d_wave"].addr, out.addr), ctx)
        times.append(device.timer_stop(ctx))
    res["launch_device_ms"] = {"median_ms": statistics.median(times[1:]), "min_ms": min(times[1:]), "max_ms": max(times[1:])}
    res["written_GBps"] = S * res["table_KB_per_sample"] / 1e6 / (res["launch_device_ms"]["median_ms"] / 1e3)

    # (b) the reference-style host build of one sample, and what the spectrum does with a host table
    def host_build(sample=samples[0]):
        dfs = [param.cloud_brewster_grey(**{k: v for k, v in d.items() if k != "kind"}) for d in sample]
        return pz.cloud_averaging(dfs)
    res["host_per_sample"] = stats_ms(host_build)
    one = host_build()
    compact = {k: np.ascontiguousarray(one[k].values.reshape(nlayer, NIN)) for k in ("opd", "w0", "g0")}

    def digest_upload():
        stack = np.concatenate([compact[k] for k in ("opd", "w0", "g0")])
        px.content_digest(grid) + px.content_digest(stack)
        device.DeviceArray.from_host(grid, ctx)
        device.DeviceArray.from_host(stack, ctx)
        device.sync(ctx)
    res["digest_upload"] = stats_ms(digest_upload)

    # (c) spectra fed from the batch against spectra fed host dictionaries of the same values
    tabs = param.cloud_tables_batch(samples[:NSPEC])
    dicts = [dict(t) for t in param.cloud_tables_batch(samples[:NSPEC])]
    dicts = [{k: d[k] for k in ("opd", "w0", "g0")} for d in dicts]      # what a host build hands over, with wavenumber=
    a = jdi.spectrum_batch([case(t) for t in tabs], opa, calculation="reflected+thermal")
    b = jdi.spectrum_batch([case(d) for d in dicts], opa, calculation="reflected+thermal")
    res["spectra_equal"] = bool(all(np.array_equal(x["albedo"], y["albedo"]) and np.array_equal(x["thermal"], y["thermal"])
                                    for x, y in zip(a, b)))

    def fed(tables):
        return lambda: jdi.spectrum_batch([case(t) for t in tables], opa, calculation="reflected+thermal")
    res["spectrum_from_batch"] = stats_ms(fed(tabs), per=NSPEC)
    res["spectrum_from_host_dicts"] = stats_ms(fed(dicts), per=NSPEC)
    res["spectra_per_run"] = NSPEC
    print(json.dumps(res))


if __name__ == "__main__":
    main()
