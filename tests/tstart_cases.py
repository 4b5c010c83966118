"""Shared by test_tstart_host.py and test_tstart_gpu.py: the cases of tests/golden/tstart.npz (outputs of the reference's
own climate.t_start, tests/golden/make_tstart.py) as arguments of picaso_amd.climate.t_start.  The opacity planes are those
of climate_fluxes.npz's scenes; tstart.npz holds the pressures in bar, the zones and what the reference did."""
import functools
import os

import numpy as np

from helpers import GOLDEN

CASES = ("one", "one_noegp", "two", "holes", "clamp", "root")


@functools.lru_cache(maxsize=None)
def fixtures():
    return np.load(os.path.join(GOLDEN, "tstart.npz")), np.load(os.path.join(GOLDEN, "climate_fluxes.npz"))


def case_calls():
    ts, _ = fixtures()
    return [(c, k) for c in CASES for k in range(int(ts[c + "/ncall"]))]


def adiabat(pc):
    ts, _ = fixtures()
    return pc.AdiabatBundle_Tuple(*[ts["adiabat/" + k] for k in pc.AdiabatBundle_Tuple._fields])


def scene_args(pc, scene, plevel, tmin=-np.inf, tmax=np.inf, t_level=None, up=lambda x: x):
    """``(Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid, F0PI), holes`` of a climate_fluxes.npz
    scene, as tests/test_climate_fluxes.py builds them; ``up`` is applied to every opacity plane."""
    _, g = fixtures()
    c = scene

    def tup(prefix):
        p = {k: up(g["%s/%s%s" % (c, prefix, k)]) for k in ("dtau", "tau", "w0", "cosb", "ftau_cld", "ftau_ray", "gcos2",
                                                           "w0_no_raman", "dtau_og", "tau_og", "w0_og", "cosb_og")}
        return (pc.OpacityWEd_Tuple(p["dtau"], p["tau"], p["w0"], p["cosb"], p["ftau_cld"], p["ftau_ray"], p["gcos2"],
                                    p["w0_no_raman"], None),
                pc.OpacityNoEd_Tuple(p["dtau_og"], p["tau_og"], p["w0_og"], p["cosb_og"]))
    nlevel, nwno, ngauss = g[c + "/tau"].shape
    t_level = g[c + "/tlevel"] if t_level is None else t_level
    atm = pc.Atmosphere_Tuple(None, None, nlevel, np.array(t_level, dtype=float), np.array(plevel, dtype=float), None, None,
                              None, None)
    wed, noed = tup("")
    sp = pc.ScatteringPhase_Tuple(np.full(nwno, 0.1), 3, 0, 1.0, -1.0, 2.0, -0.5, 1.0)
    dis = pc.Disco_Tuple(5, 1, g[c + "/gweight"], g[c + "/tweight"], g[c + "/ubar0"], g[c + "/ubar1"], 1.0)
    og = pc.Opagrid_Tuple(nwno, g[c + "/dwni"], g[c + "/wno"], ngauss, g[c + "/gauss_wts"], tmin, tmax)
    kw = {}
    if c == "holes":
        hw, hn = tup("clear/")
        kw = dict(do_holes=True, fhole=0.3, hole_OpacityWEd=hw, hole_OpacityNoEd=hn)
    return (atm, wed, noed, sp, dis, og, g[c + "/f0pi"]), kw


def run(pc, case, call, up=lambda x: x, **kw):
    """picaso_amd.climate.t_start on call `call` of `case`, restarted from the temperature the reference started from
    -> (its six values, the Atmosphere tuple it was given, the arguments of get_fluxes for that scene)."""
    ts, _ = fixtures()
    tag = "%s/%d/" % (case, call)
    (atm, wed, noed, sp, dis, og, f0pi), holes = scene_args(pc, str(ts[case + "/scene"]), ts[case + "/plevel"],
                                                          float(ts[case + "/tmin"]), float(ts[case + "/tmax"]),
                                                          ts[tag + "t_in"], up)
    conv = pc.convergence_criteriaT(*[(int if i < 2 else float)(x) for i, x in enumerate(ts["conv"])])
    out = pc.t_start(int(ts[case + "/nofczns"]), ts[case + "/nstr"], conv, float(ts[case + "/rfaci"]),
                     float(ts[case + "/rfacv"]), ts[case + "/tidal"], atm, wed, noed, sp, dis, og, adiabat(pc), f0pi, 1,
                     np.zeros(0), verbose=0, egp_stepmax=bool(ts[case + "/egp"]), **holes, **kw)
    return out, atm, ((wed, noed, sp, dis, og, f0pi), holes)
