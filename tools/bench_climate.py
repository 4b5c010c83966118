#!/usr/bin/env python
"""One inputs.climate() run at the climate tables' shape (run on the GPU box): 91 levels, 661 bins x 8 Gauss points, five
disk angles, a synthetic premixed correlated-k table (a grey-ish absorber that grows with temperature and pressure) with a
small chemistry table of three gases, no star.

Measured in ONE process with the host clock: the wall time of the whole call, the number of profile / t_start / get_fluxes /
get_nets_tbatch / calculate_atm calls (and the profiles that went through get_nets_tbatch), and the time spent inside the
three device calls -- each of them ends with its results on the host, so the host clock around it includes the device work.
``device_share`` = that time over the wall time: what is left is the host side of the driver (the Newton algebra of t_start,
the chemistry interpolation, the atmosphere set-up inside calculate_atm counts as device time here).  The second of two
runs is the one reported (the first fills the caches and compiles nothing new).  Prints one JSON object.

``--diseq``: the same run with ``climate(diseq_chem=True)`` on a synthetic ON-THE-FLY object at the same shape: a dozen per-gas
tables (ten absorbers with different spectral shapes plus H2 and He of next to no opacity, so that the mixture is normalised
by the whole gas) and a chemistry table of those gases, ``atmosphere(quench=True, mh=1, cto_relative=1)``.  Reported in
addition: the number of resort-rebin mix calls (``mix_my_opacities_gasesfly``, one per calculate_atm call) and of
update_quench_levels calls, the seconds inside the mix call -- the kernel is launched asynchronously, so the context is
synchronised before the clock is read, in this mode only -- and ``mix_share`` / ``calculate_atm_share`` of the wall time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picaso_amd import _lib  # noqa: E402
from picaso_amd import device as _device  # noqa: E402
from picaso_amd import climate as pc  # noqa: E402
from picaso_amd import justdoit as jdi  # noqa: E402
from picaso_amd import optics as px  # noqa: E402


def adiabat():
    """$picaso_refdata's table when it is set, else the copy the test fixture carries."""
    if os.environ.get("picaso_refdata"):
        return pc.load_adiabat()
    ts = np.load(os.path.join(ROOT, "tests", "golden", "tstart.npz"))
    return pc.AdiabatBundle_Tuple(*[ts["adiabat/" + k] for k in pc.AdiabatBundle_Tuple._fields])


def opacity(ctx, nwno, ngauss):
    temps = np.array([100.0, 200.0, 400.0, 800.0, 1500.0, 2500.0, 4000.0])
    press = np.array([1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3])
    wno = np.linspace(300.0, 9000.0, nwno)
    x, wg = np.polynomial.legendre.leggauss(ngauss)
    lt, lp = np.log(temps / 1000.0)[None, :, None, None], np.log(press)[:, None, None, None]
    w = (wno / 3000.0)[None, None, :, None]
    g = (0.5 * (x + 1.0))[None, None, None, :]
    ln_kappa = np.log(2.0e-26) + 1.0 * lt + 0.4 * lp - 0.8 * w + 0.5 * np.sin(7.0 * w) + 4.0 * g
    nt, npr = len(temps), len(press)
    cia_t = [75.0, 500.0, 2000.0, 6000.0]
    opa = px.RetrieveCKs(wno, 0.5 * wg, np.tile(press, nt), np.repeat(temps, npr), np.full(nt, npr), ln_kappa,
                         continuum={"H2H2": {t: np.full(nwno, 1.0e-12) for t in cia_t}}, cia_temps=cia_t,
                         rayleigh_opa={"H2": 1.0e-27 * (wno / 1.0e4) ** 4}, ctx=ctx)
    opa.delta_wno = np.abs(np.gradient(wno))
    rows_t, rows_p = np.repeat(temps, npr), np.tile(press, nt)
    h2o = 1.0e-3 * (rows_t / 1000.0) ** -0.5
    opa.full_abunds = {"pressure": rows_p, "temperature": rows_t, "H2": 0.85 - h2o, "He": np.full(rows_t.size, 0.15),
                       "H2O": h2o}
    return opa


FLY_GASES = {"H2O": (1.2e-23, 0.8, 0.0), "CH4": (1.5e-23, 0.3, 1.0), "CO": (1.0e-23, 1.5, 2.0), "NH3": (4.0e-23, -0.4, 3.0),
             "CO2": (1.0e-21, 1.0, 4.0), "HCN": (1.0e-21, 0.5, 5.0), "N2": (1.0e-27, 0.0, 0.0), "PH3": (1.0e-20, 0.7, 6.0),
             "H2S": (1.0e-22, 1.2, 7.0), "C2H2": (1.0e-20, 0.9, 8.0), "H2": (1.0e-32, 0.0, 0.0), "He": (1.0e-32, 0.0, 0.0)}


def opacity_onfly(ctx, nwno, ngauss):
    """As ``opacity``, from twelve per-gas tables mixed on the fly: gas -> (cm^2 per molecule at 1000 K and 1 bar, slope in
    wavenumber / 3000, phase of its band structure)."""
    temps = np.array([100.0, 200.0, 400.0, 800.0, 1500.0, 2500.0, 4000.0])
    press = np.array([1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3])
    wno = np.linspace(300.0, 9000.0, nwno)
    x, wg = np.polynomial.legendre.leggauss(ngauss)
    lt, lp = np.log(temps / 1000.0)[None, :, None, None], np.log(press)[:, None, None, None]
    w = (wno / 3000.0)[None, None, :, None]
    g = (0.5 * (x + 1.0))[None, None, None, :]
    kappas = {m: np.log(a) + 1.0 * lt + 0.4 * lp - s * w + 0.5 * np.sin(7.0 * w + ph) + 4.0 * g
              for m, (a, s, ph) in FLY_GASES.items()}
    nt, npr = len(temps), len(press)
    cia_t = [75.0, 500.0, 2000.0, 6000.0]
    opa = px.RetrieveCKs(wno, 0.5 * wg, np.tile(press, nt), np.repeat(temps, npr), np.full(nt, npr), kappas=kappas,
                         gauss_pts=0.5 * (x + 1.0), on_fly=True,
                         continuum={"H2H2": {t: np.full(nwno, 1.0e-12) for t in cia_t}}, cia_temps=cia_t,
                         rayleigh_opa={"H2": 1.0e-27 * (wno / 1.0e4) ** 4}, ctx=ctx)
    opa.delta_wno = np.abs(np.gradient(wno))
    rows_t, rows_p = np.repeat(temps, npr), np.tile(press, nt)
    xt, y = rows_t / 1000.0, np.log10(rows_p)
    cols = {"H2O": 1.0e-3 * xt ** -0.5, "CH4": 4.0e-4 * xt ** -2.0 * 10 ** (0.1 * y), "CO": 1.0e-4 * xt ** 2.0 * 10 ** (-0.1 * y),
            "NH3": 5.0e-5 * xt ** -2.0 * 10 ** (0.1 * y), "CO2": 1.0e-7 * xt ** 0.5, "HCN": 1.0e-8 * xt ** 1.5,
            "N2": 3.0e-5 * xt ** 0.5, "PH3": 3.0e-7 / xt, "H2S": np.full(rows_t.size, 1.0e-5), "C2H2": 1.0e-9 * xt,
            "He": np.full(rows_t.size, 0.15)}
    cols["H2"] = 1.0 - sum(cols.values())
    opa.full_abunds = dict({"pressure": rows_p, "temperature": rows_t}, **{m: cols[m] for m in FLY_GASES})
    return opa


def case(nlevel, teff, rcb, t_top):
    ad = adiabat()
    c = jdi.inputs(calculation="browndwarf")
    c.inputs["climate"] = dict(ad._asdict())
    c.setup_climate()
    c.gravity(gravity=1000.0)
    c.effective_temp(teff)
    p = np.logspace(-4, 2, nlevel)
    t = np.full(nlevel, float(t_top))
    for j in range(rcb + 1, nlevel):                             # isothermal above the guessed boundary, the adiabat below
        grad = pc.did_grad_cp(t[j - 1], np.sqrt(p[j - 1] * p[j]), ad)[0]
        t[j] = np.exp(np.log(t[j - 1]) + grad * (np.log(p[j]) - np.log(p[j - 1])))
    c.inputs_climate(temp_guess=t, pressure=p, rcb_guess=rcb, rfacv=0.0)
    return c


class Timers:
    def __init__(self):
        self.n, self.s, self.profiles = {}, {}, 0

    def wrap(self, name, timed=True):
        real = getattr(pc, name)

        def call(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            if name == "get_nets_tbatch":
                self.profiles += len(a[0])
            t0 = time.perf_counter()
            try:
                return real(*a, **k)
            finally:
                if timed:
                    self.s[name] = self.s.get(name, 0.0) + time.perf_counter() - t0
        setattr(pc, name, call)
        return real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nlevel", type=int, default=91)
    ap.add_argument("--nwno", type=int, default=661)
    ap.add_argument("--ngauss", type=int, default=8)
    ap.add_argument("--teff", type=float, default=1000.0)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--diseq", action="store_true", help="climate(diseq_chem=True) on an on-the-fly opacity object")
    args = ap.parse_args()
    ctx = _lib.context(0)
    opa = (opacity_onfly if args.diseq else opacity)(ctx, args.nwno, args.ngauss)
    rcb = (2 * args.nlevel) // 3
    out = {"shape": dict(nlevel=args.nlevel, nwno=args.nwno, ngauss=args.ngauss, nangle=5), "teff": args.teff,
           "diseq": bool(args.diseq)}
    for _ in range(args.runs):
        timers = Timers()
        saved = {n: timers.wrap(n) for n in ("get_fluxes", "get_nets_tbatch", "calculate_atm")}
        saved.update({n: timers.wrap(n, timed=False) for n in ("profile", "t_start")})
        mix = dict(n=0, s=0.0)
        real_mix = opa.mix_my_opacities_gasesfly if args.diseq else None
        try:
            c = case(args.nlevel, args.teff, rcb, 0.6 * args.teff)
            kw = {}
            if args.diseq:
                saved["update_quench_levels"] = timers.wrap("update_quench_levels", timed=False)
                c.atmosphere(df=dict(c.inputs["atmosphere"]["profile"]), quench=True, mh=1, cto_relative=1)
                kw = dict(diseq_chem=True)

                def timed_mix(*a, **k):
                    _device.sync(ctx)
                    t1 = time.perf_counter()
                    try:
                        return real_mix(*a, **k)
                    finally:
                        _device.sync(ctx)
                        mix["n"] += 1
                        mix["s"] += time.perf_counter() - t1
                opa.mix_my_opacities_gasesfly = timed_mix
            t0 = time.perf_counter()
            res = c.climate(opa, verbose=False, **kw)
            wall = time.perf_counter() - t0
        finally:
            for n, real in saved.items():
                setattr(pc, n, real)
            opa.__dict__.pop("mix_my_opacities_gasesfly", None)     # the instance attribute: the method is back
        device = sum(timers.s.values())
        out["climate"] = dict(wall_s=wall, converged=int(res["converged"]), cvz_locs=[int(x) for x in res["cvz_locs"]],
                              calls=timers.n, profiles_through_get_nets_tbatch=timers.profiles,
                              seconds_inside={k: round(v, 4) for k, v in timers.s.items()}, device_share=device / wall,
                              t_min=float(res["temperature"].min()), t_max=float(res["temperature"].max()))
        if args.diseq:
            out["climate"].update(mix_calls=mix["n"], seconds_inside_mix=round(mix["s"], 4), mix_share=mix["s"] / wall,
                                  calculate_atm_share=timers.s.get("calculate_atm", 0.0) / wall)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
