"""Shared by tests/golden/make_diseq.py (which runs the REFERENCE's climate driver with ``diseq=True``) and by
test_diseq_host.py / test_diseq_gpu.py (which run picaso_amd.climate's): the cases, the stand-in bundle, the stand-in
``calculate_atm`` and the one call that drives ``profile`` / ``find_strat`` / ``run_diseq_climate_workflow`` of either module with
the same positional arguments.  Built on climate_driver_cases.py: its scenes, ``start_profile``, ``Calls``, ``spy_t_start`` and the
indices of the returned values.

The stand-in bundle writes smooth analytic abundances ``f(T, P)`` (``equilibrium``) of H2, H2O, CO, CH4, CO2, NH3, N2, HCN and
PH3 into the profile.  Handed ``quench_levels`` it quenches in its own way -- every molecule of a name constant from the top
down to its level -- which is enough for a stand-in: what is under test is the driver, which must hand over the levels that
``update_quench_levels`` (the module's own, through ``get_quench_levels``) gives for the kzz profile and the ``Atmosphere`` of that
moment.  Every dictionary handed over is recorded.

The stand-in ``calculate_atm`` scales the layer optical depths of the scene by

    s(layer) = plane_scale(T)[layer] * (CH4[layer] / CH4_eq(1000 K, 1 bar)) ** 0.25

with ``CH4[layer]`` the mean of the two levels of the bundle's CURRENT profile, so the planes follow both the temperatures and
the quenched chemistry: a driver that forgets the refresh after quenching, or quenches at other levels, lands on other
temperatures.  ``Atmosphere.scale_height`` (cm, constant gravity ``GRAV``) and ``mmw_layer`` are filled in: ``get_quench_levels``
reads both.
"""
import collections
import functools
import os

import numpy as np

import climate_driver_cases as cd

GASES = ("H2", "H2O", "CO", "CH4", "CO2", "NH3", "N2", "HCN", "PH3")
K_B, M_P = 1.380649e-23, 1.66053906660e-27          # J/K, kg: for the stand-in's scale height only
MH = 3.0                                            # the bundle's metallicity: the CO and HCN time scales depend on it
KZ_CONST = 3.0e10                                   # cm^2/s: the constant kzz of the case without a self-consistent one


def equilibrium(t, p):
    """Smooth stand-in abundances at temperature ``t`` (K) and pressure ``p`` (bar) -> {gas: array}."""
    t, p = np.asarray(t, dtype=float), np.asarray(p, dtype=float)
    x, y = t / 1000.0, np.log10(p)
    out = {"H2O": 1.0e-3 * x ** -0.5, "CO": 5.0e-4 * x ** 0.8 * 10 ** (-0.05 * y), "CH4": 4.0e-4 * x ** -3.0 * 10 ** (0.2 * y),
           "CO2": 1.0e-7 * x ** 0.5 * 10 ** (0.1 * y), "NH3": 1.0e-5 * x ** -2.0 * 10 ** (0.15 * y),
           "N2": 6.0e-5 * x ** 0.3, "HCN": 1.0e-8 * x ** 1.5 * 10 ** (-0.1 * y), "PH3": 3.0e-7 * x ** -1.0 * 10 ** (0.05 * y)}
    out["H2"] = 0.85 - sum(out.values())
    return {k: out[k] for k in GASES}


CH4_REF = float(equilibrium(1000.0, 1.0)["CH4"])


def dict_frame(cols):
    return cols


class Bundle(cd.Bundle):
    """climate_driver_cases.Bundle with the stand-in chemistry.  ``frame``: what a profile is made of -- a dictionary of arrays
    for picaso_amd, ``pandas.DataFrame`` for the reference (whose ``update_quench_levels`` reads ``.values``).  ``n_premix`` counts
    the calls without quench levels, ``n_premix_levels`` those with; ``quench_seen`` keeps every dictionary handed over."""

    def __init__(self, nlevel, frame=dict_frame, kz=None):
        super().__init__(nlevel)
        self.frame = frame
        self.inputs["approx"]["chem_params"] = dict(quench=True, no_ph3=False, cold_trap=False, vol_rainout=False)
        self.inputs["atmosphere"]["mh"] = MH
        if kz is not None:
            self.inputs["atmosphere"]["kzz"]["constant_kzz"] = np.array(kz, dtype=float)
        self.n_premix_levels, self.quench_seen = 0, []

    def add_pt(self, T, P):
        self.n_add_pt += 1
        self.inputs["atmosphere"]["profile"] = self.frame({"temperature": np.array(T, dtype=float),
                                                           "pressure": np.array(P, dtype=float)})

    def premix_atmosphere(self, opa=None, quench_levels=None, verbose=True):
        prof = self.inputs["atmosphere"]["profile"]
        t, p = np.array(prof["temperature"], dtype=float), np.array(prof["pressure"], dtype=float)
        cols = equilibrium(t, p)
        if quench_levels is None:
            self.n_premix += 1
        else:
            self.n_premix_levels += 1
            self.quench_seen.append({k: int(v) for k, v in quench_levels.items()})
            for name, q in quench_levels.items():
                for mol in name.split("-"):
                    cols[mol][:q] = cols[mol][q]
        self.inputs["atmosphere"]["profile"] = self.frame(dict({"temperature": t, "pressure": p}, **cols))


def scaled_planes(base, t_level, ch4_level):
    """climate_driver_cases.scaled_planes with the CH4 factor of the module's docstring."""
    ch4 = np.asarray(ch4_level, dtype=float)
    s = (cd.plane_scale(t_level) * (0.5 * (ch4[:-1] + ch4[1:]) / CH4_REF) ** 0.25)[:, None, None]
    out = dict(base)
    for k, tk in (("dtau", "tau"), ("dtau_og", "tau_og")):
        out[k] = np.ascontiguousarray(base[k] * s)
        out[tk] = np.ascontiguousarray(np.concatenate((base[tk][:1], base[tk][:1] + np.cumsum(out[k], axis=0))))
    return out


def scale_height(t_level):
    """cm, at constant gravity ``cd.GRAV`` (m/s^2) and ``cd.MMW``, 3 % above what get_quench_levels would compute itself."""
    return 1.03 * K_B * np.asarray(t_level, dtype=float) / (cd.MMW * M_P * cd.GRAV) * 1e2


def make_calculate_atm(mod, base, sp, dis, calls, up=lambda x: x):
    """``calculate_atm(bundle, opacityclass, only_atmosphere=False)`` for module ``mod`` (its namedtuples)."""
    def calculate_atm(bundle, opacityclass, only_atmosphere=False):
        prof = bundle.inputs["atmosphere"]["profile"]
        t, p = np.array(prof["temperature"], dtype=float), np.array(prof["pressure"], dtype=float)
        atm = mod.Atmosphere_Tuple(cd.lapse(t, p), np.full(len(t) - 1, cd.MMW), len(t), t, p, [], np.zeros((0, len(t))), [],
                                   scale_height(t))
        if only_atmosphere:
            calls.n_atm_only += 1
            return atm
        calls.n_atm += 1
        pl = {k: up(v) for k, v in scaled_planes(base, t, np.array(prof["CH4"], dtype=float)).items()}
        wed = mod.OpacityWEd_Tuple(pl["dtau"], pl["tau"], pl["w0"], pl["cosb"], pl["ftau_cld"], pl["ftau_ray"], pl["gcos2"],
                                   pl["w0_no_raman"], None)
        noed = mod.OpacityNoEd_Tuple(pl["dtau_og"], pl["tau_og"], pl["w0_og"], pl["cosb_og"])
        return wed, noed, sp, dis, atm, (None, None)
    return calculate_atm


# name -> as climate_driver_cases.CASES; `sc_kzz`: self_consistent_kzz.  Every case runs with diseq=True.
CASES = {
    "profile_sc": dict(kind="profile", scene="a", nstr=[0, 13, 19, 0, 0, 0], nofczns=1, start=(2600.0, 13, 1.0, None, 0.15),
                       conv=(10, 7, 5.0, 5.0, 7.0), final=False, save_kzz=True, sc_kzz=True),
    "profile_const": dict(kind="profile", scene="a", nstr=[0, 13, 19, 0, 0, 0], nofczns=1, start=(2600.0, 13, 1.0, None, 0.15),
                          conv=(10, 7, 5.0, 5.0, 7.0), final=False, save_kzz=False, sc_kzz=False),
    "strat": dict(kind="find_strat", scene="a", nstr=[0, 12, 19, 0, 0, 0], nofczns=1,
                  start=(2600.0, 12, 1.0, (10, 11, 1.3), 0.15), sc_kzz=True),
    "workflow": dict(kind="workflow", scene="a", nstr=[0, 12, 19, 0, 0, 0], nofczns=1, start=(2600.0, 12, 1.0, None, 0.0),
                     sc_kzz=True),
}


def drive(mod, case, base, sp, dis, og, f0pi, adiabat, t0, pressure, tidal, calls, frame=dict_frame, **extra):
    """Run one case with module ``mod`` -> (the returned values, the final nstr, the bundle).  ``mod.calculate_atm`` and
    ``mod.t_start`` must already be the stand-in and the spy; ``extra``: ``_fluxes`` for picaso_amd."""
    c = CASES[case]
    nlevel = len(pressure)
    bundle = Bundle(nlevel, frame=frame, kz=None if c["sc_kzz"] else np.full(nlevel, KZ_CONST))
    opa = cd.Opacity(f0pi)
    cloud = cd.mod_cloud_parameters()
    nstr = list(c["nstr"])
    common = (adiabat, opa, cd.GRAV, cd.RFACI, cd.RFACV, tidal, og, cloud, 1, np.zeros(0), np.zeros(0))
    with np.errstate(all="ignore"):
        if c["kind"] == "profile":
            out = mod.profile(bundle, c["nofczns"], nstr, t0.copy(), pressure, *common, mod.convergence_criteriaT(*c["conv"]),
                              c["final"], verbose=False, save_kzz=c["save_kzz"], self_consistent_kzz=c["sc_kzz"], diseq=True,
                              **extra)
        elif c["kind"] == "find_strat":
            out = mod.find_strat(bundle, c["nofczns"], nstr, t0.copy(), pressure, cd.lapse(t0, pressure), *common, None, None,
                                 verbose=0, diseq=True, **extra)
        else:
            out = mod.run_diseq_climate_workflow(bundle, c["nofczns"], nstr, t0.copy(), pressure, *common, verbose=False,
                                                 save_kzz=True, **extra)
    return out, nstr, bundle


def outputs(case, out):
    idx = cd.PROFILE_OUT if CASES[case]["kind"] == "profile" else cd.STRAT_OUT
    return {k: np.array(out[i], dtype=float) for k, i in idx.items()}


QUENCH_NAMES = ("CO-CH4-H2O", "CO2", "NH3-N2", "HCN", "PH3")


def quench_table(seen):
    """The sequence of quench_levels dictionaries as an integer array (call, name); -1: the name is absent."""
    return np.array([[d.get(k, -1) for k in QUENCH_NAMES] for d in seen], dtype=np.int64).reshape(len(seen), len(QUENCH_NAMES))


# ---------------------------------------------------------------------------------------------------------------------
# get_quench_levels and adjust_quench_chemistry: the inputs of the cases of diseq.npz
# ---------------------------------------------------------------------------------------------------------------------
Atm = collections.namedtuple("Atm", ["t_level", "p_level", "dtdp", "mmw_layer", "scale_height"])
Q_NLEVEL, Q_GRAV, Q_MMW = 16, 1000.0, 2.3
# name -> (T top, T bottom, kz, mh_linear, PH3); kz: a number, or "varying": 1e4 over the column and one element short
QUENCH_CASES = {"hot_kz9": (400.0, 3000.0, 1e9, 1, True), "hot_kz2": (400.0, 3000.0, 1e2, 1, True),
                "hot_kz5": (400.0, 3000.0, 1e5, 1, True), "cold_extends": (150.0, 1500.0, 1e9, 1, True),
                "raises": (600.0, 900.0, 1e9, 1, True), "mh30": (400.0, 3000.0, 1e9, 30, True),
                "no_ph3": (400.0, 3000.0, 1e9, 1, False), "varying_kz": (400.0, 3000.0, "varying", 1, True)}


def quench_inputs(name):
    t0, t1, kz, mh, ph3 = QUENCH_CASES[name]
    p = np.logspace(-4, 2, Q_NLEVEL)
    t = np.exp(np.linspace(np.log(t0), np.log(t1), Q_NLEVEL))
    if kz == "varying":
        kz = np.logspace(10, 6, Q_NLEVEL - 1)
    else:
        kz = np.full(Q_NLEVEL, kz)
    # scale heights 2 % above the constant-gravity ones get_quench_levels falls back on, and only for the layers (one short
    # of the levels): the last level, and every level of an extension, keeps the fallback
    sh = 1.02 * 1.38e-23 / (Q_MMW * 1.66e-27) * t[:-1] * 1e2 / Q_GRAV
    atm = Atm(t, p, cd.lapse(t, p), np.full(Q_NLEVEL - 1, Q_MMW), sh)
    return atm, kz, mh, ph3, np.full(Q_NLEVEL, 1e-3), np.full(Q_NLEVEL, 0.85)


ADJUST_GASES = GASES + ("He",)
# name -> (T top, T bottom, quench levels or None: those of get_quench_levels at kz = 1e9, columns left out of the table)
ADJUST_CASES = {"all": (400.0, 3000.0, {"PH3": 12, "CO-CH4-H2O": 9, "CO2": 7, "NH3-N2": 10, "HCN": 4}, ()),
                "no_co2_level": (400.0, 3000.0, {"PH3": 3, "CO-CH4-H2O": 12, "NH3-N2": 13, "HCN": 14}, ()),
                "missing_molecules": (400.0, 3000.0, {"PH3": 12, "CO-CH4-H2O": 9, "CO2": 7, "NH3-N2": 10, "HCN": 4},
                                      ("PH3", "HCN", "N2")),
                "extends": (150.0, 1500.0, None, ()), "extends_no_co2": (150.0, 1500.0, {"CO-CH4-H2O": 17, "NH3-N2": 20}, ()),
                "empty": (400.0, 3000.0, {}, ())}


def adjust_table(leave_out=()):
    """A chemistry table on 7 temperatures x 13 pressures up to 3e6 bar (the extension reaches 1e6): smooth abundances of the
    gases above and He that are not bilinear in (1/T, log P); every row sums to 1."""
    temps, press = np.array([75.0, 200.0, 500.0, 1000.0, 1800.0, 3000.0, 6000.0]), np.logspace(-5, 6.5, 13)
    rows_t, rows_p = np.repeat(temps, len(press)), np.tile(press, len(temps))
    x, y = rows_t / 1000.0, np.log10(rows_p)                        # milder in 1/T than `equilibrium`: 75 K is in reach
    cols = {"H2O": 1.0e-3 * x ** -0.5, "CO": 5.0e-4 * x ** 0.8 * 10 ** (-0.05 * y), "CH4": 4.0e-4 * 10 ** (0.1 * y) / x,
            "CO2": 1.0e-7 * x ** 0.5 * 10 ** (0.1 * y), "NH3": 1.0e-5 * 10 ** (0.15 * y) / x, "N2": 6.0e-5 * x ** 0.3,
            "HCN": 1.0e-8 * x ** 1.5 * 10 ** (-0.1 * y), "PH3": 3.0e-7 * 10 ** (0.05 * y) / x,
            "He": 0.1499 * (1 + 1e-3 * y / x)}
    cols["H2"] = 1.0 - sum(cols.values())
    assert cols["H2"].min() > 0.7
    tab = {"pressure": rows_p, "temperature": rows_t}
    tab.update({k: cols[k] for k in ADJUST_GASES if k not in leave_out})
    return tab


# ---------------------------------------------------------------------------------------------------------------------
# the tests' side
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    from helpers import GOLDEN
    return np.load(os.path.join(GOLDEN, "diseq.npz"))


def run_case(pc, case, monkeypatch, fluxes=None, up=lambda x: x, spies=()):
    """picaso_amd's driver on a fixture case -> (outputs by name, the nstr list it was given, Calls, the bundle); as
    climate_driver_cases.run_case."""
    import tstart_cases as tc
    fx = fixture()
    c = CASES[case]
    base, sp, dis, og, f0pi, plevel = cd.scene_inputs(pc, c["scene"])
    calls = cd.Calls()
    calls.batches = []
    extra = {}
    if fluxes is not None:
        extra["_fluxes"] = (cd.count_fluxes(fluxes, calls), None)
    else:
        real_single, real_batched = pc.get_fluxes, pc.get_nets_tbatch

        def batched(temps, *a, **k):
            calls.n_fluxes += len(temps)
            calls.batches[-1].append(len(temps))
            return real_batched(temps, *a, **k)
        monkeypatch.setattr(pc, "get_fluxes", cd.count_fluxes(real_single, calls))
        monkeypatch.setattr(pc, "get_nets_tbatch", batched)
    real_t_start = pc.t_start

    def t_start(*a, **k):
        calls.batches.append([])
        return real_t_start(*a, **k)
    monkeypatch.setattr(pc, "calculate_atm", make_calculate_atm(pc, base, sp, dis, calls, up=up))
    monkeypatch.setattr(pc, "t_start", cd.spy_t_start(t_start, calls))
    for name, wrap in spies:
        monkeypatch.setattr(pc, name, wrap(getattr(pc, name)))
    out, nstr, bundle = drive(pc, case, base, sp, dis, og, f0pi, tc.adiabat(pc), fx[case + "/t0"], plevel, fx[case + "/tidal"],
                              calls, **extra)
    return outputs(case, out), nstr, calls, bundle


def check_against_fixture(case, out, nstr, calls, bundle):
    """What both the host and the device run must reproduce of the reference's run; prints the temperature gap first."""
    fx = fixture()
    tag = case + "/"
    assert np.array_equal(np.array(calls.nstr), fx[tag + "nstr_calls"]), (calls.nstr, fx[tag + "nstr_calls"].tolist())
    assert calls.evals == cd.expected_evals(fx[tag + "evals"]), (calls.evals, fx[tag + "evals"].tolist())
    n_tstart, _, n_atm, n_atm_only, n_add_pt, n_premix, n_premix_levels = [int(x) for x in fx[tag + "counts"]]
    assert (len(calls.nstr), calls.n_atm, calls.n_atm_only, bundle.n_add_pt, bundle.n_premix, bundle.n_premix_levels) == \
        (n_tstart, n_atm, n_atm_only, n_add_pt, n_premix, n_premix_levels)
    assert np.array_equal(quench_table(bundle.quench_seen), fx[tag + "quench_seen"]), \
        (quench_table(bundle.quench_seen).tolist(), fx[tag + "quench_seen"].tolist())
    assert list(nstr) == fx[tag + "nstr_final"].tolist()
    assert int(out["conv_flag"]) == int(fx[tag + "conv_flag"])
    gap = float(np.max(np.abs(out["temp"] - fx[tag + "temp"]) / fx[tag + "temp"]))
    print("%s: max |T - T_ref| / T_ref = %.2e, tol_temp = %.2e" % (case, gap, float(fx[tag + "tol_temp"])))
    assert gap <= float(fx[tag + "tol_temp"])
    assert out["all_profiles"].shape == fx[tag + "all_profiles"].shape
    assert out["all_kzz"].shape == fx[tag + "all_kzz"].shape
    return gap


# ---------------------------------------------------------------------------------------------------------------------
# the end-to-end run on a real opacity object that mixes per-gas correlated-k tables on the fly
# ---------------------------------------------------------------------------------------------------------------------
# gas -> (cross section scale in cm^2 per molecule at 1000 K and 1 bar, slope in wavenumber / 3000): different slopes, so that
# the mixture's spectral shape follows the abundances.  H2 and He have tables too, of next to no opacity: the resort-rebin
# mixture is normalised by the summed mixing ratio of the gases that are mixed, which must therefore be the whole gas (the
# reference's per-molecule table directory holds H2 and He for the same reason)
E2E_GASES = {"H2O": (1.2e-23, 0.8), "CH4": (1.5e-23, 0.3), "CO": (1.0e-23, 1.5), "NH3": (4.0e-23, -0.4), "CO2": (1.0e-21, 1.0),
             "H2": (1.0e-32, 0.0), "He": (1.0e-32, 0.0)}
E2E_GAUSS_PTS = np.array([0.3, 0.8])              # the abscissae of the two Gauss points of weights 0.6 and 0.4


def e2e_tables():
    """-> {gas: ln_kappa (npres, ntemp, nwno, ngauss)} growing with temperature and pressure, more opaque in the second Gauss
    point; the H2 Rayleigh cross section; a chemistry table of the five gases plus H2, He, N2 and HCN on the same (T, P)
    grid, temperature-major: CH4 and NH3 fall with temperature, CO and N2 rise, every row sums to 1."""
    e = cd.E2E
    lt, lp = np.log(e["temps"] / 1000.0)[None, :, None, None], np.log(e["press"])[:, None, None, None]
    w = (e["wno"] / 3000.0)[None, None, :, None]
    g = np.array([0.0, 1.0])[None, None, None, :]
    kappas = {m: np.log(a) + 1.0 * lt + 0.4 * lp - s * w + 2.3 * g for m, (a, s) in E2E_GASES.items()}
    rayleigh = {"H2": 1.0e-27 * (e["wno"] / 1.0e4) ** 4}
    rows_t, rows_p = np.repeat(e["temps"], len(e["press"])), np.tile(e["press"], len(e["temps"]))
    x, y = rows_t / 1000.0, np.log10(rows_p)
    cols = {"H2O": 1.0e-3 * x ** -0.5, "CH4": 4.0e-4 * x ** -2.0 * 10 ** (0.1 * y), "CO": 1.0e-4 * x ** 2.0 * 10 ** (-0.1 * y),
            "NH3": 5.0e-5 * x ** -2.0 * 10 ** (0.1 * y), "CO2": 1.0e-7 * x ** 0.5, "N2": 3.0e-5 * x ** 0.5,
            "HCN": 1.0e-8 * x ** 1.5, "He": np.full(rows_t.size, 0.15)}
    cols["H2"] = 1.0 - sum(cols.values())
    assert cols["H2"].min() > 0.7
    abunds = {"pressure": rows_p, "temperature": rows_t}
    abunds.update({k: cols[k] for k in ("H2", "He", "H2O", "CH4", "CO", "NH3", "CO2", "N2", "HCN")})
    return kappas, rayleigh, abunds


def e2e_case(jdi, px, ctx=None, kz=None):
    """-> (the inputs object after setup_climate / inputs_climate / atmosphere(quench=True, mh=1, cto_relative=1), the
    on-the-fly opacity object); as climate_driver_cases.e2e_case.  ``kz``: a Kzz column of the profile, for
    ``self_consistent_kzz=False``."""
    import tstart_cases as tc
    from picaso_amd import climate as pc
    e = cd.E2E
    kappas, rayleigh, abunds = e2e_tables()
    nt, npr = len(e["temps"]), len(e["press"])
    kw = {} if ctx is None else dict(ctx=ctx)
    cia_t = [75.0, 500.0, 2000.0, 6000.0]
    opa = px.RetrieveCKs(e["wno"], e["gauss_wts"], np.tile(e["press"], nt), np.repeat(e["temps"], npr), np.full(nt, npr),
                         kappas=kappas, gauss_pts=E2E_GAUSS_PTS, on_fly=True,
                         continuum={"H2H2": {t: np.full(len(e["wno"]), 1.0e-12) for t in cia_t}}, cia_temps=cia_t,
                         rayleigh_opa=rayleigh, **kw)
    opa.delta_wno = np.abs(np.gradient(e["wno"]))
    opa.full_abunds = abunds
    ad = tc.adiabat(pc)
    case = jdi.inputs(calculation="browndwarf")
    case.inputs["climate"] = dict(ad._asdict())
    case.setup_climate()
    case.gravity(gravity=e["gravity"])
    case.effective_temp(e["teff"])
    p = np.logspace(-4, 2, e["nlevel"])
    t = cd.start_profile(p, lambda a, b: pc.did_grad_cp(a, b, ad)[0], e["t_top"], e["rcb"])
    case.inputs_climate(temp_guess=t, pressure=p, rcb_guess=e["rcb"], rfacv=0.0)
    df = {"temperature": t.copy(), "pressure": p.copy()}
    if kz is not None:
        df["kz"] = np.array(kz, dtype=float)
    case.atmosphere(df=df, quench=True, mh=1, cto_relative=1)
    return case, opa
