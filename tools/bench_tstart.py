#!/usr/bin/env python
"""The T(P) iteration at the climate tables' shape (run on the GPU box): 91 levels x 661 bins x 8 Gauss points x 5 disk
angles, the synthetic climate scene of tools/bench_extra.py (BENCH_ONLY=climate), planes resident.

Measured in ONE process, host clock around calls that end with their results on the host (so a device synchronise):
  (a) the Jacobian's 91 perturbed profiles through get_fluxes_tbatch(nets_only=True): the per-angle level planes written,
      then summed by three more kernels;
  (b) the same profiles through get_nets_tbatch: the fused kernel of toon_lvl.hip that never writes those planes;
in alternating blocks after a warm-up of both, and one whole climate.t_start call.  (b) counts as faster only when the
gap between the block medians exceeds the spread among (a)'s own blocks.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib, disco, resident  # noqa: E402
from picaso_amd import climate as pc  # noqa: E402
from picaso_amd import synthetic as syn  # noqa: E402
from picaso_amd.device import DeviceArray  # noqa: E402


def scene(ctx, nlev=91, nw=661, ngq=8):
    """tools/bench_extra.py's climate scene, pressures in bar."""
    g, gw, t, tw = disco.get_angles_1d(5)
    u0, u1, _, _, _ = disco.compute_disco(5, 1, g, t, 0.0)
    scs = [syn.make_scene(nlev - 1, nw, seed=70 + ig, gas_scale=10.0 ** (0.5 * ig - 2)) for ig in range(ngq)]
    keys = resident.REFLECTED_PLANES + ("w0_no_raman",)
    st = {k: DeviceArray.from_host(np.ascontiguousarray(np.stack([sc[k] for sc in scs], axis=2)), ctx) for k in keys}
    _, wg = np.polynomial.legendre.leggauss(ngq)
    wno = scs[0]["wno"]
    atm = pc.Atmosphere_Tuple(None, None, nlev, np.asarray(scs[0]["tlevel"], dtype=float), scs[0]["plevel"] * 1e-6, None,
                              None, None, None)
    sp = pc.ScatteringPhase_Tuple(np.zeros(nw), 3, 0, 1.0, -1.0, 2.0, -0.5, 1.0)
    dis = pc.Disco_Tuple(5, 1, gw, tw, u0, u1, 1.0)
    og = pc.Opagrid_Tuple(nw, np.abs(np.gradient(wno)), wno, ngq, 0.5 * wg, 75.0, 4000.0)
    wed = pc.OpacityWEd_Tuple(*[st[k] for k in ("dtau", "tau", "w0", "cosb", "ftau_cld", "ftau_ray", "gcos2",
                                                "w0_no_raman")], None)
    noed = pc.OpacityNoEd_Tuple(*[st[k] for k in ("dtau_og", "tau_og", "w0_og", "cosb_og")])
    return atm, wed, noed, sp, dis, og


def adiabat():
    """$picaso_refdata's table when it is set, else the copy the test fixture carries."""
    if os.environ.get("picaso_refdata"):
        return pc.load_adiabat()
    ts = np.load(os.path.join(ROOT, "tests", "golden", "tstart.npz"))
    return pc.AdiabatBundle_Tuple(*[ts["adiabat/" + k] for k in pc.AdiabatBundle_Tuple._fields])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6, help="blocks per variant, alternating")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--nlevel", type=int, default=91)
    ap.add_argument("--nwno", type=int, default=661)
    args = ap.parse_args()
    ctx = _lib.context(0)
    atm, wed, noed, sp, dis, og = scene(ctx, args.nlevel, args.nwno)
    nlev = args.nlevel
    t0 = atm.t_level
    temps = np.stack([t0 + (np.arange(nlev) == jm) * max(1e-4 * t0[jm], 3.0) for jm in range(nlev)])
    common = (atm, wed, noed, sp, dis, og)

    def parent():
        return pc.get_fluxes_tbatch(temps, *common, ctx=ctx, chunk=nlev, nets_only=True)

    def fused():
        return pc.get_nets_tbatch(temps, *common, ctx=ctx)
    for _ in range(args.warmup):
        ra, rb = parent(), fused()
    scale = [np.abs(x).max() for x in ra]
    out = {"shape": dict(nlevel=nlev, nwno=args.nwno, ngauss=8, nangle=5, profiles=nlev),
           "max_diff_over_field_max": float(max(np.max(np.abs(a - b)) / s for a, b, s in zip(ra, rb, scale)))}
    blocks = {"parent": [], "fused": []}
    for _ in range(args.blocks):
        for name, fn in (("parent", parent), ("fused", fused)):
            ts = []
            for _ in range(args.calls):
                t1 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t1)
            blocks[name].append(1e3 * float(np.median(ts)))
    for name, b in blocks.items():
        out["jacobian_%s_ms" % name] = dict(median=float(np.median(b)), blocks=b, spread=max(b) - min(b))
    gain = out["jacobian_parent_ms"]["median"] - out["jacobian_fused_ms"]["median"]
    out["fused_is_faster"] = bool(gain > out["jacobian_parent_ms"]["spread"])
    # one whole t_start call: one radiative zone down to level 60, the adiabat below
    first = pc.get_fluxes(*common, np.ones(args.nwno), False, True, ctx=ctx)
    tidal = np.zeros(nlev) - first[5][0]
    nstr = [0, (2 * nlev) // 3, nlev - 2, 0, 0, 0]
    conv = pc.convergence_criteriaT(10, 7, 5.0, 5.0, 7.0)
    ncall = [0, 0]
    single, batched = pc.get_fluxes, pc.get_nets_tbatch

    def count_single(*a, **k):
        ncall[0] += 1
        return single(*a, ctx=ctx, **k)

    def count_batched(temps_, *a, **k):
        ncall[1] += len(temps_)
        return batched(temps_, *a, ctx=ctx, **k)
    for rep in range(2):                                      # the second call is the timed one
        ncall[:] = [0, 0]
        t1 = time.perf_counter()
        res = pc.t_start(1, nstr, conv, 1.0, 0.5, tidal, *common, adiabat(), np.ones(args.nwno), 0, np.zeros(0), verbose=0,
                         egp_stepmax=True, _fluxes=(count_single, count_batched))
        wall = time.perf_counter() - t1
    out["t_start"] = dict(s=wall, nstr=nstr, it_max=10, get_fluxes_calls=ncall[0], profiles_through_get_nets_tbatch=ncall[1],
                          t_min=float(res[0].min()), t_max=float(res[0].max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
