#!/usr/bin/env python
"""Cost of sealing a resident reflected plane set (run on the GPU box), next to what the upload costs and what a sealed
launch saves: after how many solves has a seal paid for itself?

    python tools/seal_time.py [--nwno 100000] [--nlayer 90] [--reps 5]

Prints one JSON line: upload_ms (host -> HBM of the eleven planes, once), seal_ms (picaso_reflected_planes_seal_dev:
the kernel -- nine planes read: the level checks and the clear-layer mask --, the wait for its flags, the registry; wall
clock of the call), seal_kernel_ms (HIP events around the call), solve_sealed_ms / solve_no_layer_mask_ms /
solve_all_planes_ms (steady state, the same process, PICASO_AMD_REFL_NO_LAYER_MASK / PICASO_AMD_REFL_ALL_PLANES toggled),
clear_layers (of nlayer, from the seal's mask) and break_even_solves = seal_ms / (solve_all_planes_ms - solve_sealed_ms)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib, device, disco, resident  # noqa: E402
from picaso_amd import synthetic as syn  # noqa: E402

TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nwno", type=int, default=100000)
    ap.add_argument("--nlayer", type=int, default=90)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    ctx = _lib.context(0)
    nwno, nlayer, ng = args.nwno, args.nlayer, 5
    gang, gw, tang, tw = disco.get_angles_1d(ng)
    ubar0, ubar1, _, _, _ = disco.compute_disco(ng, 1, gang, tang, 0.0)
    scene = syn.make_scene(nlayer, nwno, seed=3)
    scene["F0PI"] = np.ones(nwno)
    scene["surf_reflect"] = np.zeros(nwno)
    keys = resident.REFLECTED_PLANES + ("F0PI", "surf_reflect")
    upload, d = [], None
    for _ in range(2):                       # the second upload reuses the pooled blocks of the first
        d = None
        t0 = time.perf_counter()
        d = resident.upload_scene(scene, keys, ctx=ctx, seal=False)
        device.sync(ctx)
        upload.append((time.perf_counter() - t0) * 1e3)
    wall, ev, flags = [], [], None
    for _ in range(args.reps):
        device.sync(ctx)
        device.timer_start(ctx)
        t0 = time.perf_counter()
        flags = resident.seal_reflected_planes(ctx, nlayer + 1, nwno, d)
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(device.timer_stop(ctx))
    xint, alb = device.DeviceArray((ng, 1, nwno), ctx), device.DeviceArray((nwno,), ctx)

    def steady(knob):
        for k in ("PICASO_AMD_REFL_ALL_PLANES", "PICASO_AMD_REFL_NO_LAYER_MASK"):
            os.environ.pop(k, None)
        if knob:
            os.environ[knob] = "1"

        def step():
            resident.reflected_1d(ctx, nlayer + 1, nwno, ng, 1, d, d["surf_reflect"], ubar0, ubar1, 1.0, d["F0PI"], 3, 0,
                                  *TTHG, xint, gweight=gw, tweight=tw, albedo=alb)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.4:
            for _ in range(20):
                step()
            device.sync(ctx)
        device.timer_start(ctx)
        for _ in range(args.steps):
            step()
        return device.timer_stop(ctx) / args.steps

    h0, m0 = resident.reflected_seal_stat(ctx)[1], resident.reflected_seal_layers_stat(ctx)
    pairs = [(steady(None), steady("PICASO_AMD_REFL_ALL_PLANES"), steady("PICASO_AMD_REFL_NO_LAYER_MASK"))
             for _ in range(args.reps)]
    hits, masked = resident.reflected_seal_stat(ctx)[1] - h0, resident.reflected_seal_layers_stat(ctx) - m0
    sealed, allp = min(p[0] for p in pairs), min(p[1] for p in pairs)
    mask = resident.reflected_seal_layers(ctx, d["dtau"])
    print(json.dumps({"nwno": nwno, "nlayer": nlayer, "flags": flags, "upload_ms": [round(x, 2) for x in upload],
                      "seal_ms": [round(x, 4) for x in wall], "seal_kernel_ms": [round(x, 4) for x in ev],
                      "solve_sealed_ms": [round(p[0], 5) for p in pairs],
                      "solve_no_layer_mask_ms": [round(p[2], 5) for p in pairs],
                      "solve_all_planes_ms": [round(p[1], 5) for p in pairs],
                      "clear_layers": None if mask is None else int(mask.sum()),
                      "sealed_launches_counted": hits, "layer_mask_launches_counted": masked,
                      "break_even_solves": round(min(wall) / (allp - sealed), 1) if allp > sealed else None}), flush=True)


if __name__ == "__main__":
    main()
