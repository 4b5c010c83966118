"""Generate tests/golden/tstart.npz by running the REFERENCE's own source (build container only):

    python tests/golden/make_tstart.py

``climate.t_start`` (reference climate.py:805-1552) on the synthetic climate scenes of ``make_golden._climate_inputs``
(the planes of ``climate_fluxes.npz``'s cases ``a`` and ``holes``, which the tests read from that file), with the pressures
scaled by 1e-6 to bar so that the interior of the adiabat table is used, ``tidal = -flux_net_ir[0]`` of the starting profile
and the convergence tuple (15, 7, 5., 5., 7.).  Every case is a chain of calls, each fed the temperature the previous one
returned, as the reference's ``profile()`` drives it.

The reference is not edited: its module globals ``get_fluxes`` and ``mat_sol`` are wrapped before the call, so every
profile it evaluates (Jacobian profiles and line-search trials, in order) and every ``(A, b) -> p`` system is recorded.

Every call is then repeated from the reference's own input temperature with ``oracle.climate_oracle.get_fluxes`` in place
of the reference's ``get_fluxes`` (they agree to 1e-9 in flux).  Asserted: the same number of evaluations (if not, the scene
sits on a branch tie: change the seed, not the test).  Stored: ``gap = max |T_oracle - T_ref| / T_ref`` and
``tol_temp = max(20 gap, 1e-9)``, 20 being the ratio of the tolerances the device (2e-8) and the oracle (1e-9) are held to
against the same flux fixture (tests/test_climate_fluxes.py).

Also stored: the adiabat tables, and ``locate`` / ``did_grad_cp`` / ``convec`` samples with points off every edge of the table.
"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_shim  # noqa: E402
import make_golden as mg  # noqa: E402
from oracle import climate_oracle as co  # noqa: E402
from picaso_amd import climate as pc  # noqa: E402

cl = ref_shim.load("climate")
Opagrid = collections.namedtuple("Opagrid", ["nwno", "delta_wno", "wno", "ngauss", "gauss_wts", "tmin", "tmax"])
CONV = (15, 7, 5., 5., 7.)
NSTR_ONE, NSTR_TWO, NSTR_HOLES = [0, 12, 19, 0, 0, 0], [0, 6, 9, 9, 14, 19], [0, 9, 14, 0, 0, 0]
# name -> (scene of climate_fluxes.npz, nstr, nofczns, egp_stepmax, tmax, calls).  tmax None: below the hottest level.
# `root`: a chain that converges; its last call starts at a root and returns after one evaluation
CASES = {"one": ("a", NSTR_ONE, 1, True, 3000.0, 4), "one_noegp": ("a", NSTR_ONE, 1, False, 3000.0, 4),
         "two": ("a", NSTR_TWO, 2, True, 1.0e5, 4), "holes": ("holes", NSTR_HOLES, 1, True, 3000.0, 4),
         "clamp": ("a", NSTR_ONE, 1, True, None, 4), "root": ("a", [0, 14, 19, 0, 0, 0], 1, False, 1.0e5, 5)}
TMIN = 75.0
RFACI, RFACV = 1.0, 0.5
SHAPES = {"a": (21, 12, 3), "holes": (16, 9, 2)}


def scene(name):
    """The arguments of make_golden.make_climate_fluxes for this scene, with the reference's namedtuples."""
    nlevel, nwno, ngauss = SHAPES[name]
    sc0, st = mg._climate_inputs(nlevel, nwno, ngauss)
    geo = mg.geometry_1d(5)
    wno = sc0["wno"]
    dwni = np.abs(np.gradient(wno))
    f0pi = 0.5 + np.random.default_rng(3).random(nwno)

    def tuples(s):
        return (cl.OpacityWEd_Tuple(s["dtau"], s["tau"], s["w0"], s["cosb"], s["ftau_cld"], s["ftau_ray"], s["gcos2"],
                                    s["w0_no_raman"], None),
                cl.OpacityNoEd_Tuple(s["dtau_og"], s["tau_og"], s["w0_og"], s["cosb_og"]))
    wed, noed = tuples(st)
    sp = cl.ScatteringPhase_Tuple(np.full(nwno, 0.1), 3, 0, 1.0, -1.0, 2.0, -0.5, 1.0)
    dis = cl.Disco_Tuple(5, 1, geo["gweight"], geo["tweight"], geo["ubar0"], geo["ubar1"], 1.0)
    gw = np.array([0.5, 0.3, 0.2][:ngauss])
    gw = gw / gw.sum()
    kw = {}
    if name == "holes":
        hw, hn = tuples(mg._climate_inputs(nlevel, nwno, ngauss, cloud_scale=0.05)[1])
        kw = dict(do_holes=True, fhole=0.3, hole_OpacityWEd=hw, hole_OpacityNoEd=hn)
    return dict(nlevel=nlevel, tlevel=sc0["tlevel"].copy(), plevel=sc0["plevel"] * 1e-6, wed=wed, noed=noed, sp=sp, dis=dis,
                grid=(nwno, dwni, wno, ngauss, gw), f0pi=f0pi, kw=kw)


class Recorder:
    """Wraps the reference module's get_fluxes (or the oracle's, under the same name) and mat_sol."""

    def __init__(self, fluxes):
        self.fluxes, self.mat_sol = fluxes, cl.mat_sol
        self.profiles, self.systems = [], []

    def get_fluxes(self, Atmosphere, *a, **k):
        self.profiles.append(np.array(Atmosphere.t_level, dtype=float))
        return self.fluxes(Atmosphere, *a, **k)

    def solve(self, a, nlevel, nstrat, dflux):
        A, b = a[:nstrat, :nstrat].copy(), dflux[:nstrat].copy()
        out = self.mat_sol(a, nlevel, nstrat, dflux)
        self.systems.append((A, b, out[1][:nstrat].copy()))
        return out

    def __enter__(self):
        self.saved = (cl.get_fluxes, cl.mat_sol)
        cl.get_fluxes, cl.mat_sol = self.get_fluxes, self.solve
        return self

    def __exit__(self, *exc):
        cl.get_fluxes, cl.mat_sol = self.saved


def call(sc, adiabat, t_in, nstr, nofczns, egp, tidal, tmin, tmax, fluxes):
    """One t_start call of the reference from `t_in` -> (its six values, the recorder)."""
    atm = cl.Atmosphere_Tuple(None, None, sc["nlevel"], t_in.copy(), sc["plevel"], None, None, None, None)
    og = Opagrid(*sc["grid"], tmin, tmax)
    with Recorder(fluxes) as rec:
        with np.errstate(all="ignore"):
            out = cl.t_start(nofczns, np.array(nstr), cl.convergence_criteriaT(*CONV), RFACI, RFACV, tidal, atm, sc["wed"],
                             sc["noed"], sc["sp"], sc["dis"], og, adiabat, sc["f0pi"], 1, np.zeros(0), verbose=0,
                             egp_stepmax=egp, **sc["kw"])
    return [np.array(x, dtype=float) for x in out], rec


def samples(adiabat, store):
    rng = np.random.default_rng(11)
    tt, pt = adiabat.t_table, adiabat.p_table
    logt = np.concatenate((rng.uniform(tt[0], tt[-1], 40), [tt[0] - 0.3, tt[0], tt[1], tt[-2], tt[-1], tt[-1] + 0.2,
                                                            tt[0] - 0.3, tt[-1] + 0.2, 0.5 * (tt[0] + tt[1])]))
    logp = np.concatenate((rng.uniform(pt[0], pt[-1], 40), [pt[3], pt[0] - 1.0, pt[-1] + 1.0, pt[0], pt[-1], pt[5],
                                                            pt[-1] + 1.0, pt[0] - 1.0, 0.5 * (pt[0] + pt[1])]))
    t, p = 10.0 ** logt, 10.0 ** logp
    out = np.array([cl.did_grad_cp(a, b, adiabat) for a, b in zip(t, p)])
    store["adiabat/sample_t"], store["adiabat/sample_p"] = t, p
    store["adiabat/sample_grad"], store["adiabat/sample_cp"] = out[:, 0], out[:, 1]
    store["adiabat/locate_t"] = np.array([cl.locate(tt, x) for x in np.log10(t)])
    store["adiabat/locate_p"] = np.array([cl.locate(pt, x) for x in np.log10(p)])
    sc = scene("a")
    g, c = cl.convec(sc["tlevel"], sc["plevel"], adiabat, None)
    store["adiabat/convec_t"], store["adiabat/convec_p"] = sc["tlevel"], sc["plevel"]
    store["adiabat/convec_grad"], store["adiabat/convec_cp"] = g, c


def main():
    adiabat = pc.load_adiabat()                           # the reference's table, read as its justdoit.py:1726-1735 does
    store = {"adiabat/" + k: getattr(adiabat, k) for k in adiabat._fields}
    store["conv"] = np.array(CONV)
    samples(adiabat, store)
    ref_fluxes = cl.get_fluxes
    backtracked = clamped = False
    for name, (scn, nstr, nofczns, egp, tmax, ncall) in CASES.items():
        sc = scene(scn)
        t0 = sc["tlevel"]
        atm0 = cl.Atmosphere_Tuple(None, None, sc["nlevel"], t0.copy(), sc["plevel"], None, None, None, None)
        start = ref_fluxes(atm0, sc["wed"], sc["noed"], sc["sp"], sc["dis"], Opagrid(*sc["grid"], 0.0, 0.0), sc["f0pi"],
                           False, True, **sc["kw"])
        tidal = np.zeros(sc["nlevel"]) - start[5][0]
        clamp = tmax is None
        tmin, tmax = TMIN, (t0.max() - 25.0 if clamp else tmax)
        for k, v in dict(scene=np.array(scn), nstr=np.array(nstr), nofczns=np.array(nofczns), egp=np.array(egp),
                         rfaci=np.array(RFACI), rfacv=np.array(RFACV), tidal=tidal, plevel=sc["plevel"],
                         tmin=np.array(tmin), tmax=np.array(tmax), ncall=np.array(ncall)).items():
            store["%s/%s" % (name, k)] = v
        t_in, counts = t0, []
        calls = []
        for k in range(ncall):
            out, rec = call(sc, adiabat, t_in, nstr, nofczns, egp, tidal, tmin, tmax, ref_fluxes)
            out_o, rec_o = call(sc, adiabat, t_in, nstr, nofczns, egp, tidal, tmin, tmax, co.get_fluxes)
            assert len(rec.profiles) == len(rec_o.profiles), (name, k, len(rec.profiles), len(rec_o.profiles))
            gap = np.max(np.abs(out_o[0] - out[0]) / out[0])
            calls.append((t_in, out, rec, gap))
            counts.append(len(rec.profiles))
            n_total = len(rec.systems[0][1]) if rec.systems else 0
            # a step with more than one trial: its evaluations exceed the Jacobian's n_total + 1
            steps = len(rec.systems)
            backtracked |= steps > 0 and len(rec.profiles) - 1 > steps * (n_total + 1)
            clamped |= clamp and any(np.any(p == tmax - 0.1) for p in rec.profiles)
            t_in = out[0]
        print(name, "evaluations per call", counts, "gaps", ["%.1e" % c[3] for c in calls])
        for k, (t_in, out, rec, gap) in enumerate(calls):
            save_call(store, "%s/%d/" % (name, k), t_in, out, rec, gap)
    assert store["root/4/profiles"].shape[0] == 1 and "root/4/mat_A" not in store, "the root chain did not end at a root"
    assert backtracked, "no case backtracked in its line search"
    assert clamped, "the tmax damper never acted"
    path = os.path.join(HERE, "tstart.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def save_call(store, tag, t_in, out, rec, gap):
    store[tag + "t_in"] = t_in
    for nm, v in zip(("temp", "dtdp", "all_profiles", "flux_fourth", "flux_net_v", "flux_plus_top"), out):
        store[tag + nm] = v
    store[tag + "profiles"] = np.array(rec.profiles)
    if rec.systems:
        store[tag + "mat_A"] = np.array([s[0] for s in rec.systems])
        store[tag + "mat_b"] = np.array([s[1] for s in rec.systems])
        store[tag + "mat_p"] = np.array([s[2] for s in rec.systems])
    store[tag + "gap"] = np.array(gap)
    store[tag + "tol_temp"] = np.array(max(20.0 * gap, 1e-9))


if __name__ == "__main__":
    main()
