"""Generate tests/golden/climate_driver.npz by running the REFERENCE's own source (build container only):

    python tests/golden/make_climate_driver.py

``climate.profile``, ``find_strat``, ``run_chemeq_climate_workflow`` and ``get_kzz`` (reference climate.py) and
``fluxes.tidal_flux`` on the scenes of ``make_tstart.py``, driven through ``tests/climate_driver_cases.py``, which the tests
use to drive picaso_amd's functions the same way.  The reference is not edited: its module globals ``calculate_atm``,
``t_start``, ``get_fluxes`` and ``mat_sol`` are wrapped (``make_tstart.Recorder`` for the last two).  ``calculate_atm`` is the
stand-in of climate_driver_cases.py: the scene's planes scaled by a smooth function of the bundle's current profile.

Every case is run twice, with the reference's ``get_fluxes`` and with ``oracle.climate_oracle.get_fluxes`` in its place.
Asserted: the same ``nstr`` sequence over the ``t_start`` calls, the same number of profiles evaluated by each of them and
the same call counts (if not, the case sits on a branch tie: change its start profile).  Stored: ``gap = max |T_oracle -
T_ref| / T_ref`` of the returned profile and ``tol_temp = max(20 gap, 1e-9)``, 20 being the ratio of the tolerances the
device (2e-8) and the oracle (1e-9) are held to against the same flux fixture; asserted: ``20 gap <= 1e-4``.

``get_kzz`` and ``tidal_flux``: the reference's values, and ``tol`` = their largest relative distance from a plain numpy
re-evaluation in another operation order (below), which is what a faithful restatement may differ by.

The reference's ``justdoit`` does not import under the shims of tools/ref_shim.py (its plotting imports), so ``chem_interp`` has
no fixture here: tests/test_climate_driver_host.py checks it against scipy's RegularGridInterpolator and hand-computed indices.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
import make_tstart as mt  # noqa: E402
import climate_driver_cases as cd  # noqa: E402
from oracle import climate_oracle as co  # noqa: E402
from picaso_amd import climate as pc  # noqa: E402

cl = mt.cl
fx = ref_shim.load("fluxes")


def planes_of(sc):
    wed, noed = sc["wed"], sc["noed"]
    return dict(dtau=wed.DTAU, tau=wed.TAU, w0=wed.W0, cosb=wed.COSB, ftau_cld=wed.ftau_cld, ftau_ray=wed.ftau_ray,
                gcos2=wed.GCOS2, w0_no_raman=wed.W0_no_raman, dtau_og=noed.DTAU, tau_og=noed.TAU, w0_og=noed.W0,
                cosb_og=noed.COSB)


def run(case, sc, base, og, adiabat, t0, tidal, fluxes):
    calls = cd.Calls()
    saved = cl.calculate_atm, cl.t_start
    rec = mt.Recorder(fluxes)
    cl.calculate_atm = cd.make_calculate_atm(cl, base, sc["sp"], sc["dis"], calls)
    cl.t_start = cd.spy_t_start(saved[1], calls, count=lambda: len(rec.profiles))
    try:
        with rec, contextlib.redirect_stdout(io.StringIO()):
            out, nstr, bundle = cd.drive(cl, case, base, sc["sp"], sc["dis"], og, sc["f0pi"], adiabat, t0, sc["plevel"],
                                         tidal, calls)
    finally:
        cl.calculate_atm, cl.t_start = saved
    calls.n_fluxes = len(rec.profiles)
    return cd.outputs(case, out), nstr, calls, bundle


def driver_cases(store, adiabat):
    ref_fluxes = cl.get_fluxes
    for case, c in cd.CASES.items():
        sc = mt.scene(c["scene"])
        base = planes_of(sc)
        og = mt.Opagrid(*sc["grid"], cd.TMIN, cd.TMAX)
        t0 = cd.start_profile(sc["plevel"], lambda t, p: cl.did_grad_cp(t, p, adiabat)[0], *c["start"])
        b = cd.Bundle(len(t0))
        b.add_pt(t0, sc["plevel"])
        wed, noed, _, _, atm, _ = cd.make_calculate_atm(cl, base, sc["sp"], sc["dis"], cd.Calls())(b, None)
        start = ref_fluxes(atm, wed, noed, sc["sp"], sc["dis"], og, sc["f0pi"], False, True)
        tidal = np.zeros(len(t0)) - start[5][0]
        out, nstr, calls, bundle = run(case, sc, base, og, adiabat, t0, tidal, ref_fluxes)
        out_o, nstr_o, calls_o, _ = run(case, sc, base, og, adiabat, t0, tidal, co.get_fluxes)
        assert calls.nstr == calls_o.nstr and nstr == nstr_o, (case, calls.nstr, calls_o.nstr)
        assert calls.evals == calls_o.evals, (case, calls.evals, calls_o.evals)
        assert (calls.n_atm, calls.n_atm_only, calls.n_fluxes) == (calls_o.n_atm, calls_o.n_atm_only, calls_o.n_fluxes), case
        assert out["conv_flag"] == out_o["conv_flag"], case
        gap = float(np.max(np.abs(out_o["temp"] - out["temp"]) / out["temp"]))
        assert 20.0 * gap <= 1e-4, (case, gap)
        tag = case + "/"
        for k, v in out.items():
            store[tag + k] = v
        store[tag + "t0"], store[tag + "tidal"] = t0, tidal
        store[tag + "nstr_calls"] = np.array(calls.nstr)
        store[tag + "nstr_final"] = np.array(nstr)
        store[tag + "evals"] = np.array(calls.evals)
        store[tag + "counts"] = np.array([len(calls.nstr), calls.n_fluxes, calls.n_atm, calls.n_atm_only, bundle.n_add_pt,
                                          bundle.n_premix])
        store[tag + "gap"], store[tag + "tol_temp"] = np.array(gap), np.array(max(20.0 * gap, 1e-9))
        print("%-13s t_start %2d  get_fluxes %4d  calculate_atm %d + %d  flag %d  final nstr %s  gap %.1e"
              % (case, len(calls.nstr), calls.n_fluxes, calls.n_atm, calls.n_atm_only, int(out["conv_flag"]), nstr, gap))
    seq = store["strat_two/nstr_calls"]
    assert 2 in seq[:, 6] and seq[-1, 6] == 1, "strat_two did not find and merge a second zone"
    assert np.all(store["strat_up/nstr_calls"][:, 6] == 1) and store["strat_up/nstr_final"][1] < cd.CASES["strat_up"]["nstr"][1]
    assert store["profile_one/conv_flag"] == 1 and store["profile_one/counts"][0] < 7
    assert store["profile_itmx/conv_flag"] == 0 and store["profile_itmx/counts"][0] == 3


def kzz_alt(grav, tidal, net_layer, plus_top, adiabat, nstr, atm):
    """get_kzz in another operation order: the gas constant cancelled out of the last factor, the powers split."""
    p, t, mmw, dtdp = atm.p_level, atm.t_level, atm.mmw_layer, atm.dtdp
    nz = len(t) - 1
    r = 8.3143e7 / mmw
    pl = np.sqrt(p[1:] * p[:-1]) * 1e6
    tl = 0.5 * (t[1:] + t[:-1])
    f_sum = np.sum(plus_top)
    flx_min = abs(tidal[0]) * 0.05 ** 4
    chf = np.zeros(nz)
    chf[-1] = f_sum
    for iz in range(nz - 2, -1, -1):
        chf[iz] = max(f_sum - net_layer[iz], chf[iz + 1] * pl[iz] / (3.0 * pl[iz + 1]))
    chf = np.maximum(chf * (abs(tidal[0]) / chf[-1]), flx_min)
    floored = bool(np.any(chf == flx_min))
    grad = np.array([cl.did_grad_cp(a, b, adiabat)[0] for a, b in zip(tl, pl / 1e6)])
    h = r * tl / (grav * 1e2)
    mix = np.maximum(0.1, np.minimum(1.0, dtdp / grad))
    kz = h * mix ** (4.0 / 3.0) * np.cbrt(chf * r * tl / (3.5 * pl)) / 3.0
    kz = np.append(kz, kz[-1])
    dz = h[1:] * np.log(pl[:-1] / pl[1:])
    z = np.zeros(nz)
    z[:nz - 1] = np.cumsum(dz[:nz - 1])
    for lo, hi in ((nstr[0], nstr[1]),) + (((nstr[3], nstr[4]),) if nstr[3] != 0 else ()):
        new = []
        for i in range(lo, hi):
            ab = abs(i - np.abs(z - (z[i] + 2 * h[i])).argmin())
            be = abs(i - np.abs(z - (z[i] - 2 * h[i])).argmin())
            seg = kz[max(lo, i - ab):min(hi, i + be)]
            new.append(seg.sum() / len(seg) if len(seg) else np.nan)
        kz[lo:hi] = new
    return kz, floored


def kzz_cases(store, adiabat):
    sc = mt.scene("a")
    p = sc["plevel"]
    t = cd.start_profile(p, lambda a, b: cl.did_grad_cp(a, b, adiabat)[0], 400.0, 12, 1.0, None, 0.5)
    atm = cl.Atmosphere_Tuple(cd.lapse(t, p), np.full(len(t) - 1, cd.MMW), len(t), t, p, [], None, [], None)
    rng = np.random.default_rng(5)
    plus_top = rng.random(12) * 1e5
    f_sum = plus_top.sum()
    tidal = np.zeros(len(t)) - 0.8 * f_sum
    nets = {"floor": f_sum * (1.0 - 1e-9 * rng.random(len(t))), "nofloor": f_sum * (0.3 + 0.4 * rng.random(len(t)))}
    worst = 0.0
    store["kzz/t_level"], store["kzz/p_level"], store["kzz/plus_top"], store["kzz/tidal"] = t, p, plus_top, tidal
    for zones, nstr in (("one", [0, 12, 19, 0, 0, 0]), ("two", [0, 7, 9, 9, 14, 19])):
        for name, net in nets.items():
            with np.errstate(all="ignore"):
                kz = cl.get_kzz(cd.GRAV, tidal, net, plus_top, adiabat, nstr, atm)
                alt, floored = kzz_alt(cd.GRAV, tidal, net, plus_top, adiabat, nstr, atm)
            assert floored == (name == "floor"), (zones, name, floored)
            ok = np.isfinite(kz)
            assert np.array_equal(ok, np.isfinite(alt))
            worst = max(worst, float(np.max(np.abs(kz[ok] - alt[ok]) / np.abs(kz[ok]))))
            tag = "kzz/%s_%s/" % (zones, name)
            store[tag + "nstr"], store[tag + "net_layer"], store[tag + "kz"] = np.array(nstr), net, kz
    store["kzz/tol"] = np.array(worst)
    print("get_kzz: reference vs re-ordered numpy, max relative distance %.2e" % worst)


def tidal_alt(T_e, nlevel, pressure, col_den, inj):
    tide = -0.56687e-4 * T_e ** 4
    if inj.inject_beam:
        dep, total = np.asarray(inj.beam_profile, dtype=float)[2:], np.sum(inj.beam_profile)
    else:
        x = pressure[2:] / inj.pm
        dep, total = np.exp(1.0 + inj.hratio * np.log(x) - x ** inj.hratio) * col_den[1:], inj.wave_in
    run = np.concatenate(([0.0, 0.0], -np.cumsum(dep)))
    with np.errstate(all="ignore"):
        return tide + (run - run[-1]) * (total / run[-1])


def tidal_cases(store):
    import collections
    Inj = collections.namedtuple("InjectionBundle", ["inject_energy", "inject_beam", "wave_in", "pm", "hratio", "beam_profile"])
    p = mt.scene("a")["plevel"]
    col_den = 1e6 * (p[1:] - p[:-1]) / 1000.0
    beam = np.random.default_rng(9).random(len(p)) * 1e3
    worst = 0.0
    for name, inj in (("off", Inj(False, False, 0, 1, 1, 0)), ("chapman", Inj(True, False, 2.0e6, 0.1, 1.5, 0)),
                      ("beam", Inj(True, True, 0, 1, 1, beam))):
        out = fx.tidal_flux(700.0, len(p), p, col_den, inj)
        alt = tidal_alt(700.0, len(p), p, col_den, inj)
        worst = max(worst, float(np.max(np.abs(out - alt) / np.abs(out))))
        store["tidal/%s/out" % name] = out
        store["tidal/%s/args" % name] = np.array([float(inj.inject_energy), float(inj.inject_beam), inj.wave_in, inj.pm,
                                                    inj.hratio])
    with np.errstate(all="ignore"):
        store["tidal/two_levels/out"] = fx.tidal_flux(700.0, 2, p[:2], col_den[:1], Inj(False, False, 0, 1, 1, 0))
    store["tidal/beam_profile"], store["tidal/pressure"], store["tidal/col_den"] = beam, p, col_den
    store["tidal/tol"] = np.array(worst)
    assert np.all(store["tidal/off/out"] == -0.56687e-4 * 700.0 ** 4)
    print("tidal_flux: reference vs cumsum form, max relative distance %.2e; two levels ->" % worst,
          store["tidal/two_levels/out"])


def main():
    adiabat = pc.load_adiabat()
    store = {}
    driver_cases(store, adiabat)
    kzz_cases(store, adiabat)
    tidal_cases(store)
    path = os.path.join(HERE, "climate_driver.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
