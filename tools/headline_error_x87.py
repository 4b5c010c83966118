#!/usr/bin/env python
"""Where the 7e-10 of the headline scene comes from (run on the GPU box).

bench.py --full reports max |albedo_GPU - albedo_oracle| / albedo over all 1e5 columns of BASELINE configs[2] (7.2e-10 in
round 4) while the golden scenes sit at <= 1e-10.  This tool solves the same scene three ways -- the HIP kernel, the fp64
CPU restatement of the reference's algorithm (setup_tri_diag + tri_diag_solve, two sweeps) and the SAME restatement
compiled with long double (x87 80-bit: the reference's expressions with 11 more mantissa bits) -- and prints, for the
worst columns, which fp64 result is closer to the extended one and how close those columns come to the two-stream
singularity lambda^2 = 1/ubar0^2 of the direct-beam particular solution (fluxes.py:1155).
Writes profiles/r05_headline_error_x87.json when given -o."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as orc
from picaso_amd import _lib, device, disco, resident
from picaso_amd import synthetic as syn

TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)
nwno, nlayer, ng = int(os.environ.get("NWNO", "100000")), 90, 5
ctx = _lib.context(0)
sc = syn.make_scene(nlayer, nwno, seed=3)                     # bench.py's headline scene
gang, gw, tang, tw = disco.get_angles_1d(ng)
u0, u1, _, _, _ = disco.compute_disco(ng, 1, gang, tang, 0.0)
sc["F0PI"], sc["surf_reflect"] = np.ones(nwno), np.zeros(nwno)
d = resident.upload_scene(sc, resident.REFLECTED_PLANES + ("F0PI", "surf_reflect"), ctx=ctx)
x = device.DeviceArray((ng, 1, nwno), ctx)
alb = device.DeviceArray((nwno,), ctx)
resident.reflected_1d(ctx, nlayer + 1, nwno, ng, 1, d, d["surf_reflect"], u0, u1, 1.0, d["F0PI"], 3, 0, *TTHG, x,
                      gweight=gw, tweight=tw, albedo=alb)
xg, ag = x.to_host(), alb.to_host()
planes = [sc[k] for k in resident.REFLECTED_PLANES]
xo, _ = orc.get_reflected_1d(nlayer + 1, sc["wno"], nwno, ng, 1, *planes, 0.0, u0, u1, 1.0, np.ones(nwno), 3, 0, *TTHG)
ao = orc.compress_disco(nwno, 1.0, xo, gw, tw, np.ones(nwno))
e_alb = np.abs(ag - ao) / np.abs(ao)
e_x = np.abs(xg - xo) / np.abs(xo)
worst = np.argsort(e_alb)[::-1][:2000]
sub = [np.ascontiguousarray(p[:, worst]) for p in planes]
x80, _ = orc.get_reflected_1d(nlayer + 1, sc["wno"][worst], worst.size, ng, 1, *sub, 0.0, u0, u1, 1.0,
                              np.ones(worst.size), 3, 0, *TTHG, x80=True)
a80 = orc.compress_disco(worst.size, 1.0, x80, gw, tw, np.ones(worst.size))
g_vs_80 = np.abs(ag[worst] - a80) / np.abs(a80)
o_vs_80 = np.abs(ao[worst] - a80) / np.abs(a80)
# the singular denominator of the direct-beam term, per (layer, column, angle)
w0, fcg = sc["w0"][:, worst], (sc["ftau_cld"] * sc["cosb"])[:, worst]
sq3 = np.sqrt(3.0)
g1, g2 = (sq3 * 0.5) * (2 - w0 * (1 + fcg)), (sq3 * w0 * 0.5) * (1 - fcg)
lam2 = g1 * g1 - g2 * g2
dist = np.min(np.abs(lam2[:, :, None] - 1.0 / u0.ravel()[None, None, :] ** 2), axis=(0, 2))
out = {"scene": "bench.py headline (make_scene(90, %d, seed=3)), 5 Gauss angles" % nwno,
       "max_rel_err_albedo_gpu_vs_fp64_oracle_all_columns": float(e_alb.max()),
       "max_rel_err_xint_gpu_vs_fp64_oracle_all_columns": float(e_x.max()),
       "median_rel_err_albedo": float(np.median(e_alb)),
       "columns_above_1e-10": int((e_alb > 1e-10).sum()),
       "worst_2000_columns": {
           "gpu_vs_x87_max": float(g_vs_80.max()), "fp64_oracle_vs_x87_max": float(o_vs_80.max()),
           "gpu_closer_to_x87_in": int((g_vs_80 < o_vs_80).sum()), "of": int(worst.size),
           "gpu_vs_x87_at_the_worst_column": float(g_vs_80[0]), "oracle_vs_x87_at_the_worst_column": float(o_vs_80[0]),
           "min_abs(lambda^2 - 1/ubar0^2)_at_the_worst_column": float(dist[0]),
           "median_min_abs(lambda^2 - 1/ubar0^2)_over_the_worst_50": float(np.median(dist[:50])),
           "median_min_abs(lambda^2 - 1/ubar0^2)_over_all_2000": float(np.median(dist))}}
js = json.dumps(out, indent=1)
if "-o" in sys.argv:
    with open(sys.argv[sys.argv.index("-o") + 1], "w") as fh:
        fh.write(js + "\n")
print(js)
