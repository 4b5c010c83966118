"""Shared by tests/golden/make_climate_driver.py (which runs the REFERENCE's climate driver) and by
test_climate_driver_host.py / test_climate_driver_gpu.py (which run picaso_amd.climate's): the cases, the stand-in bundle,
the stand-in ``calculate_atm`` and the one call that drives ``profile`` / ``find_strat`` / ``run_chemeq_climate_workflow`` of
either module with the same positional arguments.

The stand-in ``calculate_atm`` returns the synthetic planes of climate_fluxes.npz with the layer optical depths scaled by

    s(layer) = (0.5 (T[layer] + T[layer + 1]) / 1000 K) ** 0.5                                     (``plane_scale``)

of the bundle's CURRENT profile, so an opacity refresh really changes the planes (a driver that refreshed them inside
``profile``'s loop, or did not refresh them between ``profile`` calls, lands on other temperatures).  ``dtau`` and ``dtau_og``
are scaled, ``tau`` and ``tau_og`` are rebuilt as their running sums from the scene's top value; every other plane is the
scene's.  The ``Atmosphere`` tuple is rebuilt from the bundle's profile: ``dtdp`` the lapse rate between levels, a mean
molecular weight of 2.3 in every layer.
"""
import collections
import functools
import os

import numpy as np

MMW = 2.3
GRAV = 10.0                                       # m/s^2: what profile / find_strat hand to get_kzz
RFACI, RFACV = 1.0, 0.0                           # no star: the brown-dwarf set-up of the climate workflow
TMIN, TMAX = 75.0, 1.0e5
PLANE_KEYS = ("dtau", "tau", "w0", "cosb", "ftau_cld", "ftau_ray", "gcos2", "w0_no_raman", "dtau_og", "tau_og", "w0_og",
              "cosb_og")


def plane_scale(t_level):
    t = np.asarray(t_level, dtype=float)
    return (0.5 * (t[:-1] + t[1:]) / 1000.0) ** 0.5


def scaled_planes(base, t_level):
    """``base``: the scene's planes by name -> the planes at this profile."""
    s = plane_scale(t_level)[:, None, None]
    out = dict(base)
    for k, tk in (("dtau", "tau"), ("dtau_og", "tau_og")):
        out[k] = np.ascontiguousarray(base[k] * s)
        out[tk] = np.ascontiguousarray(np.concatenate((base[tk][:1], base[tk][:1] + np.cumsum(out[k], axis=0))))
    return out


def lapse(temp, pressure):
    return (np.log(temp[:-1]) - np.log(temp[1:])) / (np.log(pressure[:-1]) - np.log(pressure[1:]))


def start_profile(pressure, adiabat_fn, t_top, rcb, grad_scale=1.0, bump=None, top_scale=0.0):
    """``top_scale`` x the adiabat (0: isothermal) down to level ``rcb``, then ``grad_scale`` x the adiabat:
    ``adiabat_fn(t, p) -> grad``.
    ``bump = (lo, hi, factor)``: the gradient of layers lo..hi-1 is multiplied by ``factor`` (a detached steep region)."""
    p = np.asarray(pressure, dtype=float)
    t = np.full(len(p), float(t_top))
    for j in range(1, len(p)):
        f = top_scale
        if j > rcb:
            f = grad_scale
        if bump is not None and bump[0] <= j - 1 < bump[1]:
            f = bump[2]
        g = adiabat_fn(t[j - 1], np.sqrt(p[j - 1] * p[j]))
        t[j] = np.exp(np.log(t[j - 1]) + f * g * (np.log(p[j]) - np.log(p[j - 1])))
    return t


class Bundle:
    """What profile / find_strat use of a justdoit.inputs object: ``inputs``, ``add_pt``, ``premix_atmosphere``, ``nlevel``."""

    def __init__(self, nlevel, chem_method=None):
        self.nlevel = nlevel
        self.inputs = {"approx": {"chem_method": chem_method}, "atmosphere": {"profile": None, "kzz": {}},
                       "clouds": {"do_holes": True}}          # the bundle's clouds say holes: without `cloudy` they are ignored
        self.n_add_pt = self.n_premix = 0

    def add_pt(self, T, P):
        self.n_add_pt += 1
        self.inputs["atmosphere"]["profile"] = {"temperature": np.array(T, dtype=float), "pressure": np.array(P, dtype=float)}

    def premix_atmosphere(self, opa=None, quench_levels=None, verbose=True):
        self.n_premix += 1
        prof = self.inputs["atmosphere"]["profile"]
        prof["H2"] = np.ones(len(prof["pressure"]))


class Opacity:
    def __init__(self, f0pi):
        self.relative_flux = f0pi


class Calls:
    """Counts and records what the driver did: the ``nstr`` (and ``nofczns``) of every t_start call, the number of profiles
    each of them evaluated (``evals``), the number of calculate_atm calls (full ones and atmosphere-only ones) and of
    profiles evaluated in all (``n_fluxes``)."""

    def __init__(self):
        self.nstr, self.n_atm, self.n_atm_only, self.n_fluxes, self.evals = [], 0, 0, 0, []


def make_calculate_atm(mod, base, sp, dis, calls, up=lambda x: x):
    """``calculate_atm(bundle, opacityclass, only_atmosphere=False)`` for module ``mod`` (its namedtuples)."""
    def calculate_atm(bundle, opacityclass, only_atmosphere=False):
        prof = bundle.inputs["atmosphere"]["profile"]
        t, p = prof["temperature"].copy(), prof["pressure"].copy()
        atm = mod.Atmosphere_Tuple(lapse(t, p), np.full(len(t) - 1, MMW), len(t), t, p, [], np.zeros((0, len(t))), [], None)
        if only_atmosphere:
            calls.n_atm_only += 1
            return atm
        calls.n_atm += 1
        pl = {k: up(v) for k, v in scaled_planes(base, t).items()}
        wed = mod.OpacityWEd_Tuple(pl["dtau"], pl["tau"], pl["w0"], pl["cosb"], pl["ftau_cld"], pl["ftau_ray"], pl["gcos2"],
                                   pl["w0_no_raman"], None)
        noed = mod.OpacityNoEd_Tuple(pl["dtau_og"], pl["tau_og"], pl["w0_og"], pl["cosb_og"])
        return wed, noed, sp, dis, atm, (None, None)
    return calculate_atm


def spy_t_start(t_start, calls, count=None):
    """``count()``: the number of profiles evaluated so far (default: ``calls.n_fluxes``)."""
    count = count if count is not None else (lambda: calls.n_fluxes)

    def spy(nofczns, nstr, *a, **k):
        calls.nstr.append([int(x) for x in nstr] + [int(nofczns)])
        before = count()
        out = t_start(nofczns, nstr, *a, **k)
        calls.evals.append(count() - before)
        return out
    return spy


def expected_evals(ref_evals):
    """picaso_amd's t_start evaluates what the reference's does plus one closing thermal call at the profile it returns,
    except when it returns at once from a root (one evaluation): tests/test_tstart_gpu.py."""
    return [int(n) + (0 if n == 1 else 1) for n in ref_evals]


def count_fluxes(get_fluxes, calls):
    def counted(*a, **k):
        calls.n_fluxes += 1
        return get_fluxes(*a, **k)
    return counted


# name -> what to call, the scene, the zones it starts from, and start_profile's arguments (t_top, rcb, grad_scale, bump,
# top_scale).  `conv`: the criteria of a bare profile call.  The starts are hot (2600 K at the top): there the synthetic scenes
# have smooth radiative solutions close to the start, so a chain stays short and converges.
CASES = {
    # one zone, converges at the second t_start call (before itmx = 7); kzz saved
    "profile_one": dict(kind="profile", scene="a", nstr=[0, 13, 19, 0, 0, 0], nofczns=1, start=(2600.0, 13, 1.0, None, 0.15),
                        conv=(10, 7, 5.0, 5.0, 7.0), final=False, save_kzz=True),
    # convt = 0 can never be met: runs out of itmx = 3
    "profile_itmx": dict(kind="profile", scene="holes", nstr=[0, 10, 14, 0, 0, 0], nofczns=1,
                         start=(2600.0, 10, 1.0, None, 0.0), conv=(2, 3, 5.0, 0.0, 7.0), final=True, save_kzz=False),
    "profile_two": dict(kind="profile", scene="a", nstr=[0, 9, 11, 11, 14, 19], nofczns=2,
                        start=(2600.0, 14, 1.0, (9, 12, 1.0), 0.15), conv=(8, 5, 5.0, 3.0, 7.0), final=False, save_kzz=True),
    # the start is adiabatic from level 9 down, the zone is said to start at 11: it grows upward, no second zone
    "strat_up": dict(kind="find_strat", scene="holes", nstr=[0, 11, 14, 0, 0, 0], nofczns=1,
                     start=(2600.0, 9, 1.0, None, 0.15)),
    # layer 10 of the start is 1.3 x adiabatic: a second zone at 10, grown down twice until it meets the lower one
    "strat_two": dict(kind="find_strat", scene="a", nstr=[0, 12, 19, 0, 0, 0], nofczns=1,
                      start=(2600.0, 12, 1.0, (10, 11, 1.3), 0.15)),
    # isothermal above level 12, the adiabat below
    "workflow": dict(kind="workflow", scene="a", nstr=[0, 12, 19, 0, 0, 0], nofczns=1, start=(2600.0, 12, 1.0, None, 0.0)),
}
SCENE_PRESSURE = {"a": "one/plevel", "holes": "holes/plevel"}          # keys of tstart.npz: the scenes' pressures in bar


def drive(mod, case, base, sp, dis, og, f0pi, adiabat, t0, pressure, tidal, calls, up=lambda x: x, **extra):
    """Run one case with module ``mod`` -> (the returned values, the final nstr, the bundle).  ``mod.calculate_atm`` and
    ``mod.t_start`` must already be the stand-in and the spy (the caller patches and restores them); ``extra``: ``_fluxes``
    for picaso_amd."""
    c = CASES[case]
    nlevel = len(pressure)
    bundle = Bundle(nlevel)
    opa = Opacity(f0pi)
    cloud = mod_cloud_parameters()
    nstr = list(c["nstr"])
    common = (adiabat, opa, GRAV, RFACI, RFACV, tidal, og, cloud, 1, np.zeros(0), np.zeros(0))
    with np.errstate(all="ignore"):
        if c["kind"] == "profile":
            out = mod.profile(bundle, c["nofczns"], nstr, t0.copy(), pressure, *common, mod.convergence_criteriaT(*c["conv"]),
                              c["final"], first_call_ever=True, verbose=False, save_kzz=c["save_kzz"], **extra)
        elif c["kind"] == "find_strat":
            out = mod.find_strat(bundle, c["nofczns"], nstr, t0.copy(), pressure, lapse(t0, pressure), *common, None, None,
                                 verbose=0, **extra)
        else:
            out = mod.run_chemeq_climate_workflow(bundle, c["nofczns"], nstr, t0.copy(), pressure, *common, verbose=False,
                                                  save_kzz=True, **extra)
    return out, nstr, bundle


def mod_cloud_parameters():
    return collections.namedtuple("CloudParameters", ["cloudy", "OPD", "G0", "W0"])(False, None, None, None)


# what is stored of a case's return values: name -> index in profile's list / find_strat's tuple
PROFILE_OUT = dict(conv_flag=0, temp=2, dtdp=3, flux_net_ir_layer=6, flux_net_v_layer=7, flux_plus_ir_attop=8, all_profiles=9,
                   all_kzz=11)
STRAT_OUT = dict(conv_flag=0, temp=2, dtdp=3, flux_net_ir_layer=5, flux_net_v_layer=6, flux_plus_ir_attop=7, all_profiles=10,
                 all_kzz=12)


def outputs(case, out):
    idx = PROFILE_OUT if CASES[case]["kind"] == "profile" else STRAT_OUT
    return {k: np.array(out[i], dtype=float) for k, i in idx.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the tests' side: the fixture, the scenes as climate_fluxes.npz holds them, and one run of picaso_amd's driver
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    from helpers import GOLDEN
    return np.load(os.path.join(GOLDEN, "climate_driver.npz"))


def scene_inputs(pc, scene):
    """-> base planes by name, ScatteringPhase, Disco, Opagrid (with TMIN, TMAX), F0PI, the pressures in bar."""
    import tstart_cases as tc
    ts, g = tc.fixtures()
    plevel = ts[SCENE_PRESSURE[scene]]
    (_, _, _, sp, dis, og, f0pi), _ = tc.scene_args(pc, scene, plevel, TMIN, TMAX)
    return {k: g["%s/%s" % (scene, k)] for k in PLANE_KEYS}, sp, dis, og, f0pi, plevel


def run_case(pc, case, monkeypatch, fluxes=None, up=lambda x: x, spies=()):
    """picaso_amd's driver on a fixture case -> (outputs by name, the nstr list it was given, Calls, the bundle).
    ``fluxes``: a host ``get_fluxes`` handed in as ``_fluxes=(fluxes, None)``; ``None``: the device calls, reached -- and counted
    -- through ``pc.get_fluxes`` and ``pc.get_nets_tbatch``.  ``calls.batches``: the number of profiles of every
    ``get_nets_tbatch`` call, a new list per ``t_start`` call."""
    import tstart_cases as tc
    fx = fixture()
    c = CASES[case]
    base, sp, dis, og, f0pi, plevel = scene_inputs(pc, c["scene"])
    calls = Calls()
    calls.batches = []
    extra = {}
    if fluxes is not None:
        extra["_fluxes"] = (count_fluxes(fluxes, calls), None)
    else:
        real_single, real_batched = pc.get_fluxes, pc.get_nets_tbatch

        def batched(temps, *a, **k):
            calls.n_fluxes += len(temps)
            calls.batches[-1].append(len(temps))
            return real_batched(temps, *a, **k)
        monkeypatch.setattr(pc, "get_fluxes", count_fluxes(real_single, calls))
        monkeypatch.setattr(pc, "get_nets_tbatch", batched)
    real_t_start = pc.t_start

    def t_start(*a, **k):
        calls.batches.append([])
        return real_t_start(*a, **k)
    monkeypatch.setattr(pc, "calculate_atm", make_calculate_atm(pc, base, sp, dis, calls, up=up))
    monkeypatch.setattr(pc, "t_start", spy_t_start(t_start, calls))
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
    assert calls.evals == expected_evals(fx[tag + "evals"]), (calls.evals, fx[tag + "evals"].tolist())
    n_tstart, _, n_atm, n_atm_only, n_add_pt, n_premix = [int(x) for x in fx[tag + "counts"]]
    assert (len(calls.nstr), calls.n_atm, calls.n_atm_only, bundle.n_add_pt, bundle.n_premix) == \
        (n_tstart, n_atm, n_atm_only, n_add_pt, n_premix)
    assert list(nstr) == fx[tag + "nstr_final"].tolist()
    assert int(out["conv_flag"]) == int(fx[tag + "conv_flag"])
    gap = float(np.max(np.abs(out["temp"] - fx[tag + "temp"]) / fx[tag + "temp"]))
    print("%s: max |T - T_ref| / T_ref = %.2e, tol_temp = %.2e" % (case, gap, float(fx[tag + "tol_temp"])))
    assert gap <= float(fx[tag + "tol_temp"])
    assert out["all_profiles"].shape == fx[tag + "all_profiles"].shape
    assert out["all_kzz"].shape == fx[tag + "all_kzz"].shape
    return gap


# ---------------------------------------------------------------------------------------------------------------------
# the end-to-end run on a real opacity object: a premixed correlated-k table built from arrays
# ---------------------------------------------------------------------------------------------------------------------
E2E = dict(nlevel=16, teff=1000.0, gravity=1000.0, rcb=11, t_top=600.0,
           wno=np.linspace(400.0, 6000.0, 9), gauss_wts=np.array([0.6, 0.4]),
           temps=np.array([200.0, 800.0, 2000.0, 4000.0]), press=np.array([1e-5, 1e-3, 1e-1, 1e1, 1e3]))


def e2e_tables():
    """-> ln_kappa (npres, ntemp, nwno, ngauss) of a grey-ish absorber that grows with temperature and pressure, more opaque
    in the second Gauss point and towards small wavenumbers; the H2 Rayleigh cross section; a chemistry table of three gases
    on the same (T, P) grid, temperature-major."""
    e = E2E
    lt, lp = np.log(e["temps"] / 1000.0)[None, :, None, None], np.log(e["press"])[:, None, None, None]
    w = (e["wno"] / 3000.0)[None, None, :, None]
    g = np.array([0.0, 1.0])[None, None, None, :]
    ln_kappa = np.log(2.0e-26) + 1.0 * lt + 0.4 * lp - 0.8 * w + 2.3 * g
    rayleigh = {"H2": 1.0e-27 * (e["wno"] / 1.0e4) ** 4}
    rows_t, rows_p = np.repeat(e["temps"], len(e["press"])), np.tile(e["press"], len(e["temps"]))
    h2o = 1.0e-3 * (rows_t / 1000.0) ** -0.5
    abunds = {"pressure": rows_p, "temperature": rows_t, "H2": 0.85 - h2o, "He": np.full(rows_t.size, 0.15), "H2O": h2o}
    return ln_kappa, rayleigh, abunds


def e2e_case(jdi, px, ctx=None):
    """-> (the inputs object after setup_climate / inputs_climate, the opacity object).  The adiabat tables are those of
    tstart.npz, handed in through inputs['climate'] (no reference data directory is needed)."""
    import tstart_cases as tc
    from picaso_amd import climate as pc
    e = E2E
    ln_kappa, rayleigh, abunds = e2e_tables()
    nt, npr = len(e["temps"]), len(e["press"])
    kw = {} if ctx is None else dict(ctx=ctx)
    cia_t = [75.0, 500.0, 2000.0, 6000.0]                      # a collision-induced continuum far below the table's opacity
    opa = px.RetrieveCKs(e["wno"], e["gauss_wts"], np.tile(e["press"], nt), np.repeat(e["temps"], npr), np.full(nt, npr),
                         ln_kappa, continuum={"H2H2": {t: np.full(len(e["wno"]), 1.0e-12) for t in cia_t}}, cia_temps=cia_t,
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
    t = start_profile(p, lambda a, b: pc.did_grad_cp(a, b, ad)[0], e["t_top"], e["rcb"])
    case.inputs_climate(temp_guess=t, pressure=p, rcb_guess=e["rcb"], rfacv=0.0)
    return case, opa
