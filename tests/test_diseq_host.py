"""Disequilibrium (quench) chemistry of the climate solve on the host: deq_chem.get_quench_levels, climate.update_quench_levels,
inputs.adjust_quench_chemistry / premix_atmosphere(quench_levels=) / find_kzz / add_pt / atmosphere(mh=), and
climate.profile / find_strat / run_diseq_climate_workflow with diseq=True, against tests/golden/diseq.npz (what the
reference's own functions did, tests/golden/make_diseq.py).  The flux calls are oracle.climate_oracle.get_fluxes through the
`_fluxes` injection and calculate_atm is the stand-in of diseq_cases.py, so nothing here needs a GPU."""
import collections
import contextlib
import io

import numpy as np
import pytest

import climate_driver_cases as cd
import diseq_cases as dq
import tstart_cases as tc
from picaso_amd import climate as pc
from picaso_amd import deq_chem
from picaso_amd import justdoit as jdi

EPS = 8 * 2.0 ** -53
Opa = collections.namedtuple("Opa", ["full_abunds"])
CHEM = dict(quench=True, no_ph3=False, cold_trap=False, vol_rainout=False)


@pytest.fixture(scope="module")
def fx():
    return dq.fixture()


def _levels(row):
    """A row of quench_table -> the dictionary."""
    return {k: int(v) for k, v in zip(dq.QUENCH_NAMES, row) if v >= 0}


# ---------------------------------------------------------------------------------------------------------------------
# get_quench_levels, update_quench_levels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in dq.QUENCH_CASES if n != "raises"])
def test_get_quench_levels_matches_the_reference(fx, name):
    """The same names and the same integers; t_mix within the distance the generator measured between the reference and a
    re-ordered numpy evaluation.  cold_extends continues the profile by ten levels: levels past the 16 handed in."""
    atm, kz, mh, ph3, h2o, h2 = dq.quench_inputs(name)
    levels, t_mix = deq_chem.get_quench_levels(atm, kz, dq.Q_GRAV, mh, PH3=ph3, H2O=h2o if ph3 else None, H2=h2 if ph3 else None)
    want = _levels(fx["quench/%s/levels" % name])
    assert {k: int(v) for k, v in levels.items()} == want and all(isinstance(v, (int, np.integer)) for v in levels.values())
    ref, tol = fx["quench/%s/t_mix" % name], float(fx["quench/tol_tmix"])
    assert t_mix.shape == ref.shape == ((26,) if name == "cold_extends" else (16,))
    worst = float(np.max(np.abs(t_mix - ref) / ref))
    print("%s: %s, t_mix max relative distance %.2e, tol %.2e" % (name, want, worst, tol))
    assert worst <= tol
    if name == "cold_extends":
        assert max(levels.values()) >= 16
    if name == "no_ph3":
        assert "PH3" not in levels


def test_get_quench_levels_raises_the_references_exception(fx):
    atm, kz, mh, ph3, h2o, h2 = dq.quench_inputs("raises")
    with pytest.raises(Exception) as err:
        deq_chem.get_quench_levels(atm, kz, dq.Q_GRAV, mh, PH3=ph3, H2O=h2o, H2=h2)
    assert str(err.value) == str(fx["quench/raises/raises"]) and type(err.value) is Exception


def test_oh_conc_is_the_references_formula():
    t, p = np.array([500.0, 2000.0]), np.array([1e-3, 10.0])
    want = 10 ** (3.672 - 14791 / t) * 1e-3 * 0.85 ** -0.5 * p ** -0.5 * (p * 1e6 / (1.3807e-16 * t))
    assert np.allclose(deq_chem.OH_conc(t, p, 1e-3, 0.85), want, rtol=4e-16, atol=0)


@pytest.mark.parametrize("name,cols,mh", [("with_ph3_mh3", ("H2", "H2O", "PH3"), 3), ("no_ph3_column", ("H2", "H2O"), 1),
                                          ("mh_absent", ("H2", "H2O", "PH3"), None)])
def test_update_quench_levels_matches_the_reference(fx, name, cols, mh):
    """PH3 only with H2, H2O and PH3 among the columns; mh from inputs['atmosphere'], 1 with the reference's warning without."""
    atm, kz, _, _, h2o, h2 = dq.quench_inputs("hot_kz9")
    values = {"H2": h2, "H2O": h2o, "PH3": h2o * 1e-3}
    b = collections.namedtuple("Holder", ["inputs"])({"atmosphere": {
        "profile": dict({"temperature": atm.t_level, "pressure": atm.p_level}, **{k: values[k] for k in cols})}})
    if mh is not None:
        b.inputs["atmosphere"]["mh"] = mh
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        levels = pc.update_quench_levels(b, atm, kz, dq.Q_GRAV)
    assert {k: int(v) for k, v in levels.items()} == _levels(fx["update/%s/levels" % name])
    assert out.getvalue() == str(fx["update/%s/printed" % name])
    assert ("mh was not explicitly set" in out.getvalue()) == (mh is None)


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(dq.CASES))
def test_diseq_driver_follows_the_reference(case, monkeypatch, oracle, fx):
    """The reference's zones over the t_start calls, its evaluations per call, its calculate_atm / add_pt / premix_atmosphere
    counts (with and without levels), the SEQUENCE of quench_levels dictionaries it handed to premix_atmosphere, conv_flag,
    final nstr, and the returned temperatures within tol_temp.  The planes of the stand-in calculate_atm follow the quenched
    CH4, so a driver that skipped a refresh, or took the kzz or the Atmosphere of another moment, misses the temperatures."""
    from oracle import climate_oracle as co
    out, nstr, calls, bundle = dq.run_case(pc, case, monkeypatch, fluxes=co.get_fluxes)
    dq.check_against_fixture(case, out, nstr, calls, bundle)
    kzz = bundle.inputs["atmosphere"]["kzz"]
    assert sorted(kzz.keys()) == fx[case + "/kzz_keys"].tolist()
    if dq.CASES[case]["sc_kzz"]:
        assert "constant_kzz" not in kzz and np.all(np.isfinite(kzz["sc_kzz"])) and np.all(kzz["sc_kzz"] > 0)
    else:
        assert "sc_kzz" not in kzz and np.all(kzz["constant_kzz"] == dq.KZ_CONST) and out["all_kzz"].size == 0


def test_diseq_cases_quench_inside_the_grid_and_the_levels_move(fx):
    for case in dq.CASES:
        seen = fx[case + "/quench_seen"]
        assert np.all(seen[:, 0] > 0) and np.all(seen[:, 0] < 19), case
    assert len(np.unique(fx["workflow/quench_seen"], axis=0)) > 1
    assert 2 in fx["strat/nstr_calls"][:, 6] and 2 in fx["workflow/nstr_calls"][:, 6]
    # premix_atmosphere without levels: once per calculate_atm pair before the loop and once per t_start call
    n_tstart, _, n_atm, n_atm_only, n_add_pt, n_premix, n_levels = fx["profile_sc/counts"]
    assert (n_atm, n_premix, n_levels, n_add_pt) == (2 + n_tstart, 1 + n_tstart, 1 + n_tstart, 1 + n_tstart)


def test_profile_refuses_diseq_without_the_quench_switch(monkeypatch, fx):
    """Without chem_params['quench'] premix_atmosphere ignores the levels: the run would be the equilibrium one."""
    base, sp, dis, og, f0pi, plevel = cd.scene_inputs(pc, "a")
    b = dq.Bundle(21)
    b.inputs["approx"]["chem_params"]["quench"] = False
    with pytest.raises(NotImplementedError, match="quench"):
        pc.profile(b, 1, [0, 13, 19, 0, 0, 0], fx["profile_sc/t0"], plevel, tc.adiabat(pc), cd.Opacity(f0pi), cd.GRAV, 1.0, 0.0,
                   fx["profile_sc/tidal"], og, cd.mod_cloud_parameters(), 0, np.zeros(0), np.zeros(0),
                   pc.convergence_criteriaT(2, 3, 5.0, 0.0, 7.0), False, verbose=False, diseq=True)
    assert b.n_add_pt == 0


# ---------------------------------------------------------------------------------------------------------------------
# adjust_quench_chemistry / premix_atmosphere(quench_levels=)
# ---------------------------------------------------------------------------------------------------------------------
def _climate_bundle(**chem):
    b = jdi.inputs(calculation="browndwarf")
    b.inputs["climate"] = dict(tc.adiabat(pc)._asdict())
    b.setup_climate()
    b.inputs["approx"]["chem_params"] = dict(CHEM, **chem)
    return b


def _abundances(prof):
    return [k for k in prof.keys() if k not in ("temperature", "pressure")]


def _premixed(t, p, table, levels, **chem):
    b = _climate_bundle(**chem)
    b.inputs["atmosphere"]["kzz"] = {"sc_kzz": 0}                      # as climate(diseq_chem=True) prepares it
    b.add_pt(t, p)
    with contextlib.redirect_stdout(io.StringIO()):
        b.premix_atmosphere(Opa(table), levels, verbose=False)
    return b.inputs["atmosphere"]["profile"]


@pytest.mark.parametrize("name", list(dq.ADJUST_CASES))
def test_premix_with_quench_levels_matches_the_reference(fx, name):
    """premix_atmosphere(opa, quench_levels) on the reference's side ran on a pandas profile; every column but H2 within
    8 * 2^-53 relative (each value is a copy or one or two roundings of the inputs).  H2: the reference's comes back as it
    went in, because with the pandas it ran under `df.loc[:, mol].values` is a view of the column and its `old - new` is
    zero (make_diseq.py, stored as adjust/h2_untouched); here every change is booked against H2, which is held to what that
    bookkeeping is for: the sum of the columns of every level stays what the equilibrium chemistry gave."""
    tag = "adjust/%s/" % name
    t, p, levels = fx[tag + "temperature"], fx[tag + "pressure"], _levels(fx[tag + "levels"])
    table = dq.adjust_table(tuple(fx[tag + "leave_out"].tolist()))
    prof = _premixed(t, p, table, levels)
    cols = [k[len(tag + "out/"):] for k in fx.files if k.startswith(tag + "out/")]
    assert sorted(prof.keys()) == sorted(cols) and len(prof["pressure"]) == len(p)
    assert bool(fx["adjust/h2_untouched"]) and np.array_equal(fx[tag + "out/H2"], fx[tag + "eq/H2"])
    for k in cols:
        if k == "H2":
            continue
        ref = fx[tag + "out/" + k]
        assert np.max(np.abs(prof[k] - ref) / np.abs(ref)) <= EPS, (k, np.max(np.abs(prof[k] - ref) / np.abs(ref)))
    gases = _abundances(prof)
    total, total_eq = sum(prof[k] for k in gases), sum(fx[tag + "eq/" + k] for k in gases)
    assert np.max(np.abs(total - total_eq) / total_eq) <= EPS
    if name == "empty":
        assert all(np.array_equal(prof[k], fx[tag + "eq/" + k]) for k in cols)
    else:
        assert not np.array_equal(prof["H2"], fx[tag + "eq/H2"])


# six levels written out: T, and abundances that are plain decimal numbers
HAND = {"temperature": [500.0, 700.0, 900.0, 1200.0, 1600.0, 2100.0], "pressure": [1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0],
        "H2": [0.84, 0.83, 0.82, 0.81, 0.80, 0.79], "He": [0.15, 0.15, 0.15, 0.15, 0.15, 0.15],
        "H2O": [1e-3, 2e-3, 3e-3, 4e-3, 5e-3, 6e-3], "CO": [1e-4, 2e-4, 3e-4, 4e-4, 5e-4, 6e-4],
        "CH4": [6e-4, 5e-4, 4e-4, 3e-4, 2e-4, 1e-4], "CO2": [1e-7, 2e-7, 3e-7, 4e-7, 5e-7, 6e-7],
        "NH3": [6e-5, 5e-5, 4e-5, 3e-5, 2e-5, 1e-5], "N2": [1e-5, 2e-5, 3e-5, 4e-5, 5e-5, 6e-5],
        "HCN": [1e-8, 2e-8, 3e-8, 4e-8, 5e-8, 6e-8]}
HAND_LEVELS = {"CO-CH4-H2O": 3, "CO2": 2, "NH3-N2": 4, "HCN": 1}


def test_adjust_quench_chemistry_on_a_hand_worked_profile():
    """Levels 0 .. q + 1 inclusive take the value of level q (the reference's label slice df.loc[0:q+1]); CO2 is the kinetic
    fCO2 = CO H2O / (K H2) at every level, of the quenched CO and H2O and the ENTRY H2, with levels 0 .. q - 1 holding
    fCO2[q]; H2 takes up every change."""
    b = _climate_bundle()
    b.inputs["atmosphere"]["profile"] = {k: np.array(v) for k, v in HAND.items()}
    b.adjust_quench_chemistry(dict(HAND_LEVELS))
    prof = b.inputs["atmosphere"]["profile"]
    assert list(prof.keys()) == list(HAND.keys())
    assert prof["H2O"].tolist() == [4e-3] * 5 + [6e-3] and prof["CO"].tolist() == [4e-4] * 5 + [6e-4]
    assert prof["CH4"].tolist() == [3e-4] * 5 + [1e-4]
    assert prof["NH3"].tolist() == [2e-5] * 6 and prof["N2"].tolist() == [5e-5] * 6
    assert prof["HCN"].tolist() == [2e-8] * 3 + [4e-8, 5e-8, 6e-8]
    assert prof["He"].tolist() == HAND["He"] and prof["temperature"].tolist() == HAND["temperature"]
    T, h2_entry = np.array(HAND["temperature"]), np.array(HAND["H2"])
    K = 18.3 * np.exp(-2376 / T - (932 / T) ** 2)
    fco2 = prof["CO"] * prof["H2O"] / (K * h2_entry)
    fco2[:2] = fco2[2]
    assert np.max(np.abs(prof["CO2"] - fco2) / fco2) <= EPS
    assert prof["CO2"][0] == prof["CO2"][1] == prof["CO2"][2] and prof["CO2"][3] != prof["CO2"][2]
    gases = _abundances(prof)
    total, total_in = sum(prof[k] for k in gases), sum(np.array(HAND[k]) for k in gases)
    assert np.max(np.abs(total - total_in) / total_in) <= EPS
    # built with the running H2 instead, fCO2[2] (which levels 0 and 1 hold too) would differ by ~1e-3, far above EPS
    assert abs(prof["H2"][2] - h2_entry[2]) / h2_entry[2] > 1e-4


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_adjust_quench_chemistry_invariants_on_random_profiles(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(8, 24))
    t, p = np.sort(rng.uniform(300.0, 2500.0, n)), np.logspace(-4, 2, n)
    gases = list(dq.ADJUST_GASES) + ["Na"]
    entry = {"temperature": t, "pressure": p}
    entry.update({k: (0.8 if k == "H2" else 10 ** rng.uniform(-8, -3)) * (1 + rng.random(n)) for k in gases})
    levels = {k: int(rng.integers(1, n - 1)) for k in dq.QUENCH_NAMES}
    if seed % 2:
        del levels["CO2"]
    b = _climate_bundle()
    b.inputs["atmosphere"]["profile"] = {k: v.copy() for k, v in entry.items()}
    b.adjust_quench_chemistry(dict(levels))
    prof = b.inputs["atmosphere"]["profile"]
    total, total_in = sum(prof[k] for k in gases), sum(entry[k] for k in gases)
    assert np.max(np.abs(total - total_in) / total_in) <= EPS             # every change is booked against H2
    for name, q in levels.items():
        for mol in name.split("-"):
            if mol == "CO2":
                continue
            assert np.all(prof[mol][:q + 2] == entry[mol][q]) and np.array_equal(prof[mol][q + 2:], entry[mol][q + 2:]), mol
    if "CO2" not in levels:
        assert np.array_equal(prof["CO2"], entry["CO2"])
    for k in ("He", "Na", "temperature", "pressure"):                     # not in the quench sequence
        assert np.array_equal(prof[k], entry[k])


def test_adjust_quench_chemistry_extends_a_cold_profile_and_returns_the_original_length(fx):
    """A level past the grid: the top of the returned profile holds the table's chemistry at that level of the profile
    continued by ten levels along the lapse rate of the last layer."""
    tag = "adjust/extends_no_co2/"
    t, p, levels = fx[tag + "temperature"], fx[tag + "pressure"], _levels(fx[tag + "levels"])
    assert levels == {"CO-CH4-H2O": 17, "NH3-N2": 20}
    table = dq.adjust_table()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b = _climate_bundle()
        b.inputs["atmosphere"]["kzz"] = {"sc_kzz": 0}
        b.add_pt(t, p)
        b.premix_atmosphere(Opa(table), levels, verbose=False)
    prof = b.inputs["atmosphere"]["profile"]
    assert "Extending atmosphere profile deeper" in out.getvalue() and all(len(v) == 16 for v in prof.values())
    dtdp = (np.log(t[-2]) - np.log(t[-1])) / (np.log(p[-2]) - np.log(p[-1]))
    pe = np.append(p, np.logspace(np.log10(p[-1] + 100), 6, 10))
    te = t.copy()
    for i in range(16, 26):
        te = np.append(te, np.exp(np.log(te[i - 1]) - dtdp * (np.log(pe[i - 1]) - np.log(pe[i]))))
    deep = _premixed(te, pe, table, None)
    for mol, q in (("CO", 17), ("CH4", 17), ("H2O", 17), ("NH3", 20), ("N2", 20)):
        assert np.all(prof[mol] == deep[mol][q]), mol
    assert np.array_equal(prof["HCN"], deep["HCN"][:16])


def test_premix_without_levels_or_without_the_switch_is_the_equilibrium_chemistry():
    """quench_levels=None (whatever the switch says), the switch off (whatever the levels say) and an empty dictionary:
    bit for bit what chem_interp alone gives."""
    t, p = np.exp(np.linspace(np.log(400.0), np.log(3000.0), 16)), np.logspace(-4, 2, 16)
    table = dq.adjust_table()
    b = _climate_bundle(quench=False)
    b.add_pt(t, p)
    b.chem_interp(table)
    want = b.inputs["atmosphere"]["profile"]
    levels = {"CO-CH4-H2O": 9, "CO2": 7, "NH3-N2": 10}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b2 = _climate_bundle()
        b2.inputs["atmosphere"]["kzz"] = {"sc_kzz": 0}
        b2.add_pt(t, p)
        b2.premix_atmosphere(Opa(table), {}, verbose=True)
    assert "nothing has quenched" in out.getvalue()
    for got in (_premixed(t, p, table, None), _premixed(t, p, table, None, quench=False),
                _premixed(t, p, table, levels, quench=False), b2.inputs["atmosphere"]["profile"]):
        assert list(got.keys()) == list(want.keys()) and all(np.array_equal(got[k], want[k]) for k in want)
    quenched = _premixed(t, p, table, levels)
    assert not np.array_equal(quenched["CH4"], want["CH4"])
    no_ph3 = _premixed(t, p, table, levels, no_ph3=True)               # no_ph3 comes after the quench
    assert np.all(no_ph3["PH3"] == 0) and np.array_equal(no_ph3["CH4"], quenched["CH4"])
    for key in ("vol_rainout", "cold_trap"):
        with pytest.raises(NotImplementedError, match=key):
            _premixed(t, p, table, levels, **{key: True})
    # the quench switch without any Kzz (no kzz dictionary, no kz column) cannot be honoured and is refused, levels or not;
    # a kz column of the profile is a Kzz
    for lv in (None, levels):
        b3 = _climate_bundle()
        b3.add_pt(t, p)
        with pytest.raises(NotImplementedError, match="quench"):
            b3.premix_atmosphere(Opa(table), lv, verbose=False)
    b3.inputs["atmosphere"]["profile"]["kz"] = np.full(16, 1e9)
    b3.premix_atmosphere(Opa(table), levels, verbose=False)
    assert np.array_equal(b3.inputs["atmosphere"]["profile"]["CH4"], quenched["CH4"])


# ---------------------------------------------------------------------------------------------------------------------
# find_kzz, add_pt, atmosphere(mh=), climate(diseq_chem=True)
# ---------------------------------------------------------------------------------------------------------------------
def test_find_kzz_precedence():
    b = _climate_bundle()
    p, t = np.logspace(-4, 2, 6), np.linspace(300.0, 1500.0, 6)
    b.add_pt(t, p)
    assert b.find_kzz() is None
    b.inputs["atmosphere"]["profile"]["kz"] = np.full(6, 3.0)
    assert np.array_equal(b.find_kzz(), np.full(6, 3.0))
    b.inputs["atmosphere"]["kzz"] = {}
    assert np.array_equal(b.find_kzz(), np.full(6, 3.0))
    b.inputs["atmosphere"]["kzz"]["sc_kzz"] = np.full(6, 2.0)
    assert np.array_equal(b.find_kzz(), np.full(6, 2.0))
    b.inputs["atmosphere"]["kzz"]["constant_kzz"] = np.full(6, 1.0)
    assert np.array_equal(b.find_kzz(), np.full(6, 1.0))


def test_add_pt_keeps_kz_and_drops_everything_else():
    b = _climate_bundle()
    p, t = np.logspace(-4, 2, 6), np.linspace(300.0, 1500.0, 6)
    kz = np.logspace(9, 7, 6)
    b.atmosphere(df={"pressure": p, "temperature": t, "H2": np.full(6, 0.85), "H2O": np.full(6, 1e-3), "kz": kz})
    b.add_pt(t + 10.0, p)
    prof = b.inputs["atmosphere"]["profile"]
    assert list(prof.keys()) == ["temperature", "pressure", "kz"] and np.array_equal(prof["kz"], kz)
    assert np.array_equal(prof["temperature"], t + 10.0)
    b.add_pt((t + 20.0)[::-1], p[::-1])                                # reordered with the pressures
    prof = b.inputs["atmosphere"]["profile"]
    assert np.array_equal(prof["pressure"], p) and np.array_equal(prof["kz"], kz[::-1])
    b.add_pt(t[:4], p[:4])                                             # another grid: a kz of the old length cannot follow
    assert list(b.inputs["atmosphere"]["profile"].keys()) == ["temperature", "pressure"]


def test_atmosphere_takes_mh_and_cto_in_a_climate_setup_only():
    p, t = np.logspace(-4, 2, 6), np.linspace(300.0, 1500.0, 6)
    df = {"pressure": p, "temperature": t, "H2": np.full(6, 0.85)}
    b = _climate_bundle()
    b.atmosphere(df=dict(df), quench=True, mh=3, cto_relative=1)
    atm = b.inputs["atmosphere"]
    assert atm["mh"] == 3 and atm["cto_relative"] == 1 and atm["cto_absolute"] == 0.549
    assert b.inputs["approx"]["chem_params"]["quench"] is True
    b.atmosphere(df=dict(df), mh=10, cto_absolute=0.549)
    assert atm["mh"] == 10 and atm["cto_relative"] == 1.0
    with pytest.raises(Exception, match="cto_relative or cto_absolute was not"):
        b.atmosphere(df=dict(df), mh=3)
    with pytest.raises(Exception, match="cto is not an acceptance argument"):
        b.atmosphere(df=dict(df), mh=3, cto=1)
    for kw in (dict(chem_method="visscher"), dict(photochem_init_args={})):
        with pytest.raises(Exception, match="outside this package"):
            b.atmosphere(df=dict(df), **kw)
    plain = jdi.inputs(calculation="browndwarf")
    with pytest.raises(Exception, match="outside this package"):
        plain.atmosphere(df=dict(df), mh=3, cto_relative=1)
    plain.atmosphere(df=dict(df))
    assert "mh" not in plain.inputs["atmosphere"]


class _PremixedOpa:
    """What climate() reads of an opacity object before it starts; `on_fly` as given (None: absent)."""

    def __init__(self, on_fly):
        self.wno = np.linspace(500.0, 5000.0, 9)
        self.delta_wno, self.nwno = np.abs(np.gradient(self.wno)), 9
        self.temps, self.ngauss, self.gauss_wts, self.relative_flux = np.array([200.0, 800.0, 4000.0]), 2, np.array([0.6, 0.4]), None
        if on_fly is not None:
            self.on_fly = on_fly


def _ready():
    b = _climate_bundle()
    b.effective_temp(900.0)
    b.gravity(gravity=1000.0)
    p, t = np.logspace(-4, 2, 16), np.linspace(300.0, 1500.0, 16)
    b.inputs_climate(temp_guess=t, pressure=p, rcb_guess=11, rfacv=0.0)
    return b, p, t


@pytest.mark.parametrize("on_fly", [None, False])
def test_climate_diseq_refuses_an_opacity_object_that_does_not_mix_on_the_fly(on_fly):
    b, _, _ = _ready()
    with pytest.raises(Exception, match="resortrebin") as err:
        b.climate(_PremixedOpa(on_fly), diseq_chem=True, verbose=False)
    assert "premixed" in str(err.value) and "kzz" not in b.inputs["atmosphere"]


@pytest.mark.parametrize("sc_kzz", [True, False])
def test_climate_diseq_hands_the_diseq_workflow_what_the_reference_does(monkeypatch, sc_kzz):
    """need_kzz = diseq_chem or save_all_kzz: the kzz dictionary is prepared without save_all_kzz too; the workflow is
    run_diseq_climate_workflow with the equilibrium one's arguments; interpret_run says which Kzz the chemistry uses."""
    b, p, t = _ready()
    kz = np.logspace(9, 7, 16)
    prof = {"pressure": p, "temperature": t, "H2": np.full(16, 0.85)}
    if not sc_kzz:
        prof["kz"] = kz
    b.atmosphere(df=prof, quench=True, mh=1, cto_relative=1)
    seen = {}

    def workflow(bundle, nofczns, nstr, temp, pressure, adiabat, opa, grav, rfaci, rfacv, tidal, og, cloud, save_profile,
                 all_profiles, all_opd, **kw):
        seen.update(kw=kw, kzz=dict(bundle.inputs["atmosphere"]["kzz"]), grav=grav)
        net = np.linspace(1.0, 2.0, 16)
        return 1, pressure, temp + 1.0, np.ones(15), nstr, net, np.zeros(16), np.ones(9), {"pressure": pressure}, np.nan, \
            all_profiles, all_opd, np.zeros(3)

    def equilibrium(*a, **k):
        raise AssertionError("the equilibrium workflow was called")
    monkeypatch.setattr(pc, "run_diseq_climate_workflow", workflow)
    monkeypatch.setattr(pc, "run_chemeq_climate_workflow", equilibrium)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = b.climate(_PremixedOpa(True), diseq_chem=True, self_consistent_kzz=sc_kzz, verbose=True)
    assert seen["kw"] == dict(verbose=True, moist=False, save_kzz=False, self_consistent_kzz=sc_kzz) and seen["grav"] == 10.0
    if sc_kzz:
        assert seen["kzz"] == {"sc_kzz": 0} and "self-consistent" in out.getvalue()
    else:
        assert list(seen["kzz"]) == ["constant_kzz"] and np.array_equal(seen["kzz"]["constant_kzz"], kz)
        assert "constant" in out.getvalue()
    assert res["converged"] == 1 and "all_kzz" not in res
    if not sc_kzz:
        b2, _, _ = _ready()
        with pytest.raises(Exception, match="no kzz profile"):
            b2.climate(_PremixedOpa(True), diseq_chem=True, self_consistent_kzz=False, verbose=False)
