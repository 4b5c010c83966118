"""The climate driver on the host: picaso_amd.climate.profile / find_strat / run_chemeq_climate_workflow / get_kzz,
fluxes.tidal_flux and the justdoit.inputs methods of a climate run, against tests/golden/climate_driver.npz (what the
reference's own functions did, tests/golden/make_climate_driver.py).  The flux calls are oracle.climate_oracle.get_fluxes
through the `_fluxes` injection and calculate_atm is the stand-in of climate_driver_cases.py, so nothing here needs a GPU."""
import collections

import numpy as np
import pytest

import climate_driver_cases as cd
import tstart_cases as tc
from picaso_amd import climate as pc
from picaso_amd import fluxes as pf
from picaso_amd import justdoit as jdi

Inj = collections.namedtuple("InjectionBundle", ["inject_energy", "inject_beam", "wave_in", "pm", "hratio", "beam_profile"])


@pytest.fixture(scope="module")
def fx():
    return cd.fixture()


@pytest.mark.parametrize("case", list(cd.CASES))
def test_driver_follows_the_reference(case, monkeypatch, oracle):
    """The reference's sequence of zones over the t_start calls, its evaluations per call (plus this package's closing
    call), its calculate_atm / add_pt / premix_atmosphere counts, conv_flag and final nstr; the returned temperatures within
    the fixture's tol_temp.  The planes of the stand-in calculate_atm follow the profile, so a driver that refreshed the
    opacities inside profile's loop (or not between profile calls) would miss both the counts and the temperatures."""
    from oracle import climate_oracle as co
    out, nstr, calls, bundle = cd.run_case(pc, case, monkeypatch, fluxes=co.get_fluxes)
    cd.check_against_fixture(case, out, nstr, calls, bundle)
    if cd.CASES[case]["kind"] == "profile" and cd.CASES[case]["save_kzz"]:
        assert np.array_equal(bundle.inputs["atmosphere"]["kzz"]["sc_kzz"], out["all_kzz"][:len(out["temp"])])


def test_find_strat_cases_take_the_branches_they_are_named_for(fx):
    two, up = fx["strat_two/nstr_calls"], fx["strat_up/nstr_calls"]
    assert 2 in two[:, 6] and two[-1, 6] == 1                          # found a second zone, merged it
    assert np.all(up[:, 6] == 1) and up[-1, 1] < cd.CASES["strat_up"]["nstr"][1]
    assert 2 in fx["workflow/nstr_calls"][:, 6]
    assert int(fx["profile_one/conv_flag"]) == 1 and int(fx["profile_itmx/conv_flag"]) == 0


def test_profile_leaves_the_callers_arrays_alone_and_find_strat_changes_nstr(monkeypatch, oracle):
    from oracle import climate_oracle as co
    t0 = cd.fixture()["strat_up/t0"].copy()
    out, nstr, calls, _ = cd.run_case(pc, "strat_up", monkeypatch, fluxes=co.get_fluxes)
    assert np.array_equal(t0, cd.fixture()["strat_up/t0"])
    assert nstr != cd.CASES["strat_up"]["nstr"]                         # the list handed in was grown in place


def _kzz_atm(fx):
    t, p = fx["kzz/t_level"], fx["kzz/p_level"]
    return pc.Atmosphere_Tuple(cd.lapse(t, p), np.full(len(t) - 1, cd.MMW), len(t), t, p, [], None, [], None)


@pytest.mark.parametrize("name", ["one_floor", "one_nofloor", "two_floor", "two_nofloor"])
def test_get_kzz_matches_the_reference(fx, name):
    """One and two radiative zones, the minimum-flux floor active and not: within the distance the generator measured
    between the reference and a re-ordered numpy evaluation (equal bits if that was zero); NaNs (an empty averaging window)
    where the reference has them."""
    tag = "kzz/%s/" % name
    with np.errstate(all="ignore"):
        kz = pc.get_kzz(cd.GRAV, fx["kzz/tidal"], fx[tag + "net_layer"], fx["kzz/plus_top"], tc.adiabat(pc),
                        fx[tag + "nstr"].tolist(), _kzz_atm(fx))
    want, tol = fx[tag + "kz"], float(fx["kzz/tol"])
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(kz), ok)
    worst = float(np.max(np.abs(kz[ok] - want[ok]) / np.abs(want[ok])))
    print("%s: max relative distance %.2e, tol %.2e" % (name, worst, tol))
    if tol == 0.0:
        assert np.array_equal(kz[ok], want[ok])
    else:
        assert worst <= tol
    with pytest.raises(NotImplementedError, match="moist"):
        pc.get_kzz(cd.GRAV, fx["kzz/tidal"], fx[tag + "net_layer"], fx["kzz/plus_top"], tc.adiabat(pc), [0, 12, 19, 0, 0, 0],
                   _kzz_atm(fx), moist=True)


def test_update_kzz_computes_the_fluxes_it_is_not_given(fx):
    tag = "kzz/one_nofloor/"
    seen = []

    def single(atm, *a, **k):
        seen.append((a[-2], a[-1], k))
        out = [None] * 8
        out[4], out[6] = fx[tag + "net_layer"], fx["kzz/plus_top"][None, :]
        return out
    with np.errstate(all="ignore"):
        kz = pc.update_kzz(cd.GRAV, fx["kzz/tidal"], tc.adiabat(pc), [0, 12, 19, 0, 0, 0], _kzz_atm(fx), verbose=False,
                           _fluxes=(single, None))
        given = pc.update_kzz(cd.GRAV, fx["kzz/tidal"], tc.adiabat(pc), [0, 12, 19, 0, 0, 0], _kzz_atm(fx), verbose=False,
                              flux_net_ir_layer=fx[tag + "net_layer"], flux_plus_ir_attop=fx["kzz/plus_top"],
                              _fluxes=(single, None))
    assert seen == [(False, True, {})]                                 # one thermal call, no holes
    assert np.array_equal(kz, given, equal_nan=True)


@pytest.mark.parametrize("name", ["off", "chapman", "beam"])
def test_tidal_flux_matches_the_reference(fx, name):
    a = fx["tidal/%s/args" % name]
    inj = Inj(bool(a[0]), bool(a[1]), a[2], a[3], a[4], fx["tidal/beam_profile"] if a[1] else 0)
    p = fx["tidal/pressure"]
    out = pf.tidal_flux(700.0, len(p), p, fx["tidal/col_den"], inj)
    want, tol = fx["tidal/%s/out" % name], float(fx["tidal/tol"])
    worst = float(np.max(np.abs(out - want) / np.abs(want)))
    print("%s: max relative distance %.2e, tol %.2e" % (name, worst, tol))
    if tol == 0.0:
        assert np.array_equal(out, want)
    else:
        assert worst <= tol
    if name == "off":
        assert np.all(out == -0.56687e-4 * 700.0 ** 4) and not np.isnan(out).any()


def test_tidal_flux_two_levels_and_chapman(fx):
    """Two levels leave nothing deposited: 0 * 0 / 0, NaN exactly where the reference has it.  chapman peaks at 1."""
    p = fx["tidal/pressure"]
    with np.errstate(all="ignore"):
        out = pf.tidal_flux(700.0, 2, p[:2], fx["tidal/col_den"][:1], Inj(False, False, 0, 1, 1, 0))
    assert np.array_equal(np.isnan(out), np.isnan(fx["tidal/two_levels/out"])) and np.isnan(out).all()
    assert pf.chapman(0.3, 0.3, 1.7) == 1.0
    assert pf.chapman(np.array([0.1, 0.3, 1.0]), 0.3, 1.7).argmax() == 1


# ---------------------------------------------------------------------------------------------------------------------
# chem_interp.  The reference's justdoit does not import under the generator's shims, so: scipy on a rectangular table,
# hand-computed indices for the clamps.
# ---------------------------------------------------------------------------------------------------------------------
def _table(temps, press, nc_p):
    """Temperature-major ragged table: the first nc_p[it] pressures per temperature; three species, smooth but NOT bilinear
    in (1/T, log P), so the wrong cell gives another value."""
    rows_t = np.concatenate([[t] * n for t, n in zip(temps, nc_p)])
    rows_p = np.concatenate([press[:n] for n in nc_p])
    x, y = 1.0 / rows_t, np.log10(rows_p)
    return {"pressure": rows_p, "temperature": rows_t, "H2": 10 ** (-0.1 - 20.0 * x + 0.01 * y),
            "H2O": 10 ** (-3.0 + 300.0 * x - 0.2 * y + 40.0 * x * y + 3.0e4 * x * x),
            "CH4": 10 ** (-4.0 + 500.0 * x + 0.3 * y + 0.03 * y * y)}


def _bundle(t, p):
    b = jdi.inputs(calculation="browndwarf")
    b.add_pt(t, p)
    return b


def test_chem_interp_is_bilinear_in_inverse_temperature_and_log_pressure():
    from scipy.interpolate import RegularGridInterpolator
    temps, press = np.array([300.0, 500.0, 900.0, 1500.0, 2400.0]), np.logspace(-5, 2, 8)
    tab = _table(temps, press, [8] * 5)
    rng = np.random.default_rng(2)
    # below the table's third-last pressure: from there on the reference holds the lower index at nc_p - 3 (next test)
    t, p = rng.uniform(300.0, 2400.0, 30), np.sort(10 ** rng.uniform(-5, 1, 30))
    b = _bundle(t, p)
    b.chem_interp(tab)
    prof = b.inputs["atmosphere"]["profile"]
    order = np.argsort(1.0 / temps)
    for sp in ("H2", "H2O", "CH4"):
        grid = np.log10(tab[sp]).reshape(5, 8)[order]
        interp = RegularGridInterpolator(((1.0 / temps)[order], np.log10(press)), grid)
        want = 10 ** interp(np.stack([1.0 / t, np.log10(p)], axis=1))
        assert np.max(np.abs(prof[sp] - want) / want) < 1e-12, sp
    assert list(prof.keys()) == ["temperature", "pressure", "H2", "H2O", "CH4"]
    # a DataFrame is read the same way
    import pandas as pd
    b2 = _bundle(t, p)
    b2.chem_interp(pd.DataFrame(tab))
    assert all(np.array_equal(b2.inputs["atmosphere"]["profile"][k], prof[k]) for k in prof)


def test_chem_interp_clamps_off_the_table_and_at_the_ragged_edge():
    """Level 0 colder than the table, level 1 hotter, level 2 above the last pressure of its (ragged) upper column, level 3
    below the first pressure: the reference's indices by hand, the values by the bilinear form at those indices (so the
    off-table levels extrapolate, as the reference's do)."""
    temps, press = np.array([300.0, 500.0, 900.0, 1500.0]), np.logspace(-4, 2, 7)
    nc_p = [7, 7, 5, 4]                                                # hotter columns end earlier
    tab = _table(temps, press, nc_p)
    t = np.array([200.0, 2000.0, 700.0, 400.0])
    p = np.array([1e-2, 1e-1, 50.0, 1e-6])
    order = np.argsort(p)
    b = _bundle(t, p)                                                  # add_pt sorts by pressure
    b.chem_interp(tab)
    prof = b.inputs["atmosphere"]["profile"]
    t, p = t[order], p[order]
    assert np.array_equal(prof["pressure"], p)
    # by hand, per level in the sorted order (p = 1e-6, 1e-2, 1e-1, 50): t_low, then p_low = min(found, nc_p[t_low + 1] - 3)
    #   400 K, 1e-6: t_low 0 (300 < 400 < 500); no table pressure <= 1e-6 -> 0
    #   200 K, 1e-2: below the table -> t_low 0; p index 2, nc_p[1] - 3 = 4 -> 2
    #   2000 K, 1e-1: last temperature -> ntemp - 2 = 2; p index 3, nc_p[3] - 3 = 1 -> 1
    #   700 K, 50:   t_low 1 (500 < 700 < 900); p index 5, nc_p[2] - 3 = 2 -> 2
    t_low, p_low = np.array([0, 0, 2, 1]), np.array([0, 2, 1, 2])
    start = np.concatenate(([0], np.cumsum(nc_p)))
    ti = (1 / t - 1 / temps[t_low]) / (1 / temps[t_low + 1] - 1 / temps[t_low])
    pi = (np.log10(p) - np.log10(press[p_low])) / (np.log10(press[p_low + 1]) - np.log10(press[p_low]))
    assert ti[1] < 0 and ti[2] > 1 and pi[3] > 1 and pi[0] < 0            # every clamp is exercised
    for sp in ("H2", "H2O", "CH4"):
        la = np.log10(tab[sp])
        want = 10 ** ((1 - ti) * (1 - pi) * la[start[t_low] + p_low] + ti * (1 - pi) * la[start[t_low + 1] + p_low]
                      + ti * pi * la[start[t_low + 1] + p_low + 1] + (1 - ti) * pi * la[start[t_low] + p_low + 1])
        assert np.max(np.abs(prof[sp] - want) / want) < 1e-13, sp


# ---------------------------------------------------------------------------------------------------------------------
# the inputs methods and the error paths
# ---------------------------------------------------------------------------------------------------------------------
def _climate_bundle():
    b = jdi.inputs(calculation="browndwarf")
    ad = tc.adiabat(pc)
    b.inputs["climate"] = dict(ad._asdict())                           # no $picaso_refdata needed: the tables are handed in
    b.setup_climate()
    return b


def test_setup_and_inputs_climate_write_what_the_reference_writes():
    with pytest.raises(Exception, match="climate"):
        jdi.inputs(climate=True)
    with pytest.raises(Exception, match="setup_climate"):
        jdi.inputs(climate=True)
    b = _climate_bundle()
    assert b.inputs["calculation"] == "climate" and b.inputs["approx"]["rt_params"]["common"]["raman"] == 2
    assert b.inputs["disco"]["num_gangle"] == 5 and b.inputs["disco"]["num_tangle"] == 1      # 10 Gauss angles, halved
    assert np.array_equal(b.inputs["climate"]["t_table"], tc.adiabat(pc).t_table)
    p, t = np.logspace(-4, 2, 16), np.linspace(300.0, 1500.0, 16)
    with pytest.raises(Exception, match="Need to specify Teff"):
        b.inputs_climate(temp_guess=t, pressure=p, rcb_guess=11, rfacv=0.0)
    b.effective_temp(900)
    with pytest.raises(Exception, match="Need to specify gravity"):
        b.inputs_climate(temp_guess=t, pressure=p, rcb_guess=11, rfacv=0.0)
    b.gravity(gravity=1000.0)
    b.inputs_climate(temp_guess=t, pressure=p, rcb_guess=11, rfacv=0.0)
    cl = b.inputs["climate"]
    assert cl["nstr"] == [0, 11, 14, 0, 0, 0] and cl["nofczns"] == 1 and cl["rfaci"] == 1 and cl["rfacv"] == 0.0
    assert cl["moistgrad"] is False and cl["guess_temp"] is not t and np.array_equal(cl["guess_temp"], t)
    assert b.inputs["planet"]["T_eff"] == 900 and b.nlevel == 16
    assert list(b.inputs["atmosphere"]["profile"].keys()) == ["temperature", "pressure"]
    b.T_eff()
    assert b.inputs["planet"]["T_eff"] == 0
    b.add_pt(t[::-1], p[::-1])                                         # sorted by pressure
    assert np.array_equal(b.inputs["atmosphere"]["profile"]["pressure"], p)
    assert np.array_equal(b.inputs["atmosphere"]["profile"]["temperature"], t)
    with pytest.raises(Exception, match="setup_climate"):
        jdi.inputs(calculation="browndwarf").inputs_climate(temp_guess=t, pressure=p, rcb_guess=11)


def test_premix_atmosphere_and_its_limits():
    temps, press = np.array([300.0, 900.0, 2400.0]), np.logspace(-5, 2, 8)
    tab = dict(_table(temps, press, [8] * 3), PH3=np.full(24, 1e-6))
    opa = collections.namedtuple("Opa", ["full_abunds"])(tab)
    b = _climate_bundle()
    b.add_pt(np.linspace(400.0, 2000.0, 6), np.logspace(-4, 1, 6))
    b.premix_atmosphere(opa, verbose=False)
    prof = b.inputs["atmosphere"]["profile"]
    assert np.allclose(prof["PH3"], 1e-6) and b.inputs["approx"]["chem_method"] == "chemistry table loaded through opannection"
    b.atmosphere(df=dict(prof), no_ph3=True)                           # a climate set-up takes the chemistry switches
    b.premix_atmosphere(opa=opa, verbose=False)
    assert np.all(b.inputs["atmosphere"]["profile"]["PH3"] == 0)
    for key in ("quench", "vol_rainout", "cold_trap"):
        b.inputs["approx"]["chem_params"] = dict(quench=False, no_ph3=False, cold_trap=False, vol_rainout=False)
        b.inputs["approx"]["chem_params"][key] = True
        with pytest.raises(NotImplementedError, match=key):
            b.premix_atmosphere(opa, verbose=False)
    b.inputs["approx"]["chem_params"][key] = False
    b.inputs["approx"]["chem_method"] = None
    with pytest.raises(Exception, match="is not valid"):
        b.premix_atmosphere(None)
    for method, what in (("visscher_1060", "visscher"), ("photochem", "photochem")):
        b.inputs["approx"]["chem_method"] = method
        with pytest.raises(NotImplementedError, match=what):
            b.premix_atmosphere(opa)


def test_everything_out_of_scope_says_so():
    b = _climate_bundle()
    b.effective_temp(900)
    b.gravity(gravity=1000.0)
    p, t = np.logspace(-4, 2, 16), np.linspace(300.0, 1500.0, 16)
    with pytest.raises(NotImplementedError, match="pressure_grid"):
        b.add_pt(t, P_config={"n": 3})
    with pytest.raises(NotImplementedError):
        b.pressure_grid({})
    with pytest.raises(NotImplementedError, match="virga"):
        b.virga(["H2O"], "dir")
    with pytest.raises(NotImplementedError):
        b.chemeq_visscher_2121(1.0, 0.0)
    with pytest.raises(NotImplementedError, match="photochem"):
        b.premix_atmosphere_photochem()
    with pytest.raises(Exception, match="inputs_climate"):
        b.climate(None)
    b.inputs_climate(temp_guess=t, pressure=p, rcb_guess=11, rfacv=0.0)
    with pytest.raises(NotImplementedError, match="diseq"):
        b.climate(None, diseq_chem=True, verbose=False)
    with pytest.raises(NotImplementedError, match="HDF5"):
        b.climate(None, save_all_profiles="out.h5", verbose=False)
    b.inputs["climate"]["cloudy"] = True
    with pytest.raises(NotImplementedError, match="virga"):
        b.climate(None, verbose=False)
    # profile's own refusals
    fx = cd.fixture()
    base, sp, dis, og, f0pi, plevel = cd.scene_inputs(pc, "holes")
    args = (cd.Bundle(16), 1, [0, 10, 14, 0, 0, 0], fx["profile_itmx/t0"], plevel, tc.adiabat(pc), cd.Opacity(f0pi), cd.GRAV, 1.0,
            0.0, fx["profile_itmx/tidal"], og)
    tail = (0, np.zeros(0), np.zeros(0), pc.convergence_criteriaT(2, 3, 5.0, 0.0, 7.0), False)
    clear = cd.mod_cloud_parameters()
    with pytest.raises(NotImplementedError, match="virga"):
        pc.profile(*args, clear._replace(cloudy=True), *tail, verbose=False)
    with pytest.raises(NotImplementedError, match="quench"):
        pc.profile(*args, clear, *tail, verbose=False, diseq=True)
    with pytest.raises(NotImplementedError, match="moist"):
        pc.profile(*args, clear, *tail, verbose=False, moist=True)
    with pytest.raises(NotImplementedError, match="photochem"):
        pc.profile(cd.Bundle(16, chem_method="photochem"), *args[1:], clear, *tail, verbose=False)


@pytest.mark.parametrize("limit,start", [(5, 5), (3, 12)])
def test_find_strat_stops_a_zone_that_reaches_the_top(monkeypatch, limit, start):
    """The two ValueErrors: the first growth may not pass level 5, the grow phase not level 3.  profile is replaced by one
    that returns an everywhere super-adiabatic lapse rate, so the zone keeps growing; for the second, the first loop is
    left at once (the entry profile is isothermal above the zone) and one steep layer at 10 opens a second zone."""
    fx = cd.fixture()
    base, sp, dis, og, f0pi, plevel = cd.scene_inputs(pc, "a")
    ad = tc.adiabat(pc)
    grad = lambda t, p: pc.did_grad_cp(t, p, ad)[0]                    # noqa: E731
    if limit == 5:
        t0 = cd.start_profile(plevel, grad, 2600.0, 0, 1.2)            # 1.2 x adiabatic everywhere: grows from the entry profile
    else:
        t0 = cd.start_profile(plevel, grad, 2600.0, start, 1.0, (10, 11, 1.3))
    n_calls = []

    def steep_profile(bundle, nofczns, nstr, temp, pressure, *a, **k):
        n_calls.append(list(nstr))
        return [1, pressure, temp, np.full(len(temp) - 1, 5.0), a[7], np.nan, None, None, None, a[9], a[10], []]
    monkeypatch.setattr(pc, "profile", steep_profile)
    monkeypatch.setattr(pc, "calculate_atm", cd.make_calculate_atm(pc, base, sp, dis, cd.Calls()))
    nstr = [0, start, 19, 0, 0, 0]
    with pytest.raises(ValueError, match="Top of atmosphere"):
        pc.find_strat(cd.Bundle(21), 1, nstr, t0, plevel, None, ad, cd.Opacity(f0pi), cd.GRAV, 1.0, 0.0, fx["strat_two/tidal"],
                      og, cd.mod_cloud_parameters(), 0, np.zeros(0), np.zeros(0), None, None, verbose=0)
    assert nstr[1] == limit - 1
    if limit == 3:
        assert n_calls[0][3] == 10                                     # the second zone was opened before the grow phase


class _Opa:
    """What climate() itself reads of an opacity object."""

    def __init__(self, temps):
        self.wno = np.linspace(500.0, 5000.0, 9)
        self.delta_wno, self.nwno = np.abs(np.gradient(self.wno)), 9
        self.temps, self.ngauss, self.gauss_wts, self.relative_flux = np.asarray(temps), 2, np.array([0.6, 0.4]), None


@pytest.mark.parametrize("teff,tmin,tmax", [(900.0, 140.0, 5200.0), (250.0, 10, 5200.0), (2000.0, 140.0, 10000)])
def test_climate_hands_the_workflow_what_the_reference_does(monkeypatch, teff, tmin, tmax):
    """The arguments of run_chemeq_climate_workflow and the dictionary made of what it returns, with the workflow itself
    replaced: the opacity grid's temperature range widened by 30 % with the two Teff switches, no star (rfacv = 0, F0PI = 1),
    tidal = -sigma Teff^4 at every level, cloud-free CloudParameters, gravity in m/s^2, the reference's keys."""
    b = _climate_bundle()
    b.effective_temp(teff)
    b.gravity(gravity=1000.0)
    p, t = np.logspace(-4, 2, 16), np.linspace(300.0, 1500.0, 16)
    b.inputs_climate(temp_guess=t, pressure=p, rcb_guess=11, rfacv=0.5)          # rfacv is overruled: there is no star
    seen = {}

    def workflow(bundle, nofczns, nstr, temp, pressure, adiabat, opa, grav, rfaci, rfacv, tidal, og, cloud, save_profile,
                 all_profiles, all_opd, **kw):
        seen.update(locals())
        net = np.linspace(1.0, 2.0, 16)
        return 1, pressure, temp + 1.0, np.ones(15), nstr, net, np.zeros(16), np.ones(9), {"pressure": pressure}, np.nan, \
            all_profiles, all_opd, np.zeros(3)
    monkeypatch.setattr(pc, "run_chemeq_climate_workflow", workflow)
    opa = _Opa([200.0, 800.0, 4000.0])
    out = b.climate(opa, save_all_profiles=True, save_all_kzz=True, verbose=False)
    og = seen["og"]
    assert (og.tmin, og.tmax) == (tmin, tmax) and og.nwno == 9 and og.ngauss == 2
    assert seen["bundle"] is b and seen["nofczns"] == 1 and seen["nstr"] == [0, 11, 14, 0, 0, 0]
    assert seen["rfacv"] == 0.0 and seen["rfaci"] == 1 and seen["grav"] == 10.0 and seen["save_profile"] == 1
    assert np.array_equal(opa.relative_flux, np.ones(9))
    assert np.all(seen["tidal"] == -0.56687e-4 * teff ** 4)
    assert seen["cloud"].cloudy is False and seen["cloud"].OPD.shape == (15, 9, 4)
    assert seen["kw"] == dict(verbose=False, moist=False, save_kzz=True, self_consistent_kzz=True)
    assert np.array_equal(seen["all_profiles"], t) and np.array_equal(seen["all_opd"], np.zeros(15))
    assert b.inputs["atmosphere"]["kzz"] == {"sc_kzz": 0}
    assert set(out) == {"pressure", "temperature", "ptchem_df", "dtdp", "cvz_locs", "flux_ir_attop", "fnet/fnetir", "converged",
                        "flux_balance", "all_profiles", "all_opd", "all_kzz"}
    fb = out["flux_balance"]
    assert np.array_equal(fb["flux_net"], fb["flux_net_ir"] + fb["tidal"]) and out["converged"] == 1
    assert np.array_equal(out["fnet/fnetir"], fb["flux_net"] / fb["flux_net_ir"]) and np.array_equal(out["temperature"], t + 1.0)
    assert "all_kzz" not in b.climate(opa, verbose=False)
