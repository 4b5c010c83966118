"""The climate driver on the device: picaso_amd.climate.find_strat and run_chemeq_climate_workflow through the real device
calls (get_fluxes, get_nets_tbatch) against tests/golden/climate_driver.npz, the residency of the opacity planes over a whole
find_strat run, and inputs.climate() end to end on a real correlated-k opacity object."""
import ctypes
import gc

import numpy as np
import pytest

import climate_driver_cases as cd
from picaso_amd import climate as pc
from picaso_amd import justdoit as jdi
from picaso_amd import optics as px
from picaso_amd.device import DeviceArray

pytestmark = pytest.mark.gpu
TOLF = 5e-3                                        # t_start's tolf


@pytest.fixture(scope="module")
def ctx():
    return pc._lib.context()


def _n_unknowns(row):
    """The unknowns of t_start for one recorded ``nstr + [nofczns]``: the levels of the radiative zones."""
    nstr, nofczns = row[:6], row[6]
    return nstr[1] + 1 + (nstr[4] - nstr[3] if nofczns == 2 else 0)


@pytest.mark.parametrize("case", ["strat_two", "workflow"])
def test_driver_on_the_device_follows_the_reference(ctx, case, monkeypatch):
    """The 21 x 12 x 3 scene through get_fluxes / get_nets_tbatch: the reference's zones over the t_start calls, its
    evaluations per call, its call counts, temperatures within tol_temp.  The last Jacobian of the run is one batch of as
    many profiles as the final zones have unknowns (more than one: a degenerate one-unknown run cannot pass for this)."""
    def up(x):
        return DeviceArray.from_host(np.ascontiguousarray(x), ctx)
    out, nstr, calls, bundle = cd.run_case(pc, case, monkeypatch, up=up)
    cd.check_against_fixture(case, out, nstr, calls, bundle)
    last = [b for b in calls.batches if b][-1]                        # the last t_start call that took a Newton step
    which = [i for i, b in enumerate(calls.batches) if b][-1]
    n_total = last[0]                                                  # its first batched call is the Jacobian
    assert n_total >= 2 and n_total == _n_unknowns(calls.nstr[which])


def _mem(ctx):
    o = (ctypes.c_size_t * 6)()
    pc._lib.check(pc._lib.load().picaso_ctx_mem_stats(ctx, o), ctx)
    return int(o[0]), int(o[1])


def _cache(ctx):
    """Bytes and blocks of the bounded cache of per-wavelength vectors (climate._VEC_CACHE): allowed its fill."""
    vals = list(pc._VEC_CACHE.values())
    return sum(v.nbytes for v in vals), len(vals)


def test_planes_stay_resident_and_device_memory_stays_flat(ctx, monkeypatch):
    """Around the two-zone find_strat case: what the context has handed out after the whole run equals the reading after the
    first profile call (the bounded vector cache taken out of both), and no plane of calculate_atm is ever copied to the host
    -- only the flux results get_fluxes / get_nets_tbatch themselves copy back."""
    planes, copies, readings = [], [], []

    def up(x):
        d = DeviceArray.from_host(np.ascontiguousarray(x), ctx)
        planes.append((d.addr, d.addr + d.nbytes))
        return d

    def root(d):
        while hasattr(d, "_owner"):
            d = d._owner
        return d
    for name in ("to_host", "to_host_async"):
        def spy(self, *a, _real=getattr(DeviceArray, name), **k):
            copies.append(self.addr)
            copies.append(root(self).addr)
            return _real(self, *a, **k)
        monkeypatch.setattr(DeviceArray, name, spy)

    def reading(profile):
        def wrapped(*a, **k):
            out = profile(*a, **k)
            if not readings:
                gc.collect()
                readings.append((_mem(ctx), _cache(ctx)))
            return out
        return wrapped
    out, nstr, calls, bundle = cd.run_case(pc, "strat_two", monkeypatch, up=up, spies=(("profile", reading),))
    del out, bundle
    gc.collect()
    (mem0, cache0), mem1, cache1 = readings[0], _mem(ctx), _cache(ctx)
    print("after the first profile call: live %s, cache %s; after find_strat: live %s, cache %s" % (mem0, cache0, mem1, cache1))
    assert calls.n_atm >= 4 and len(planes) == 12 * calls.n_atm
    assert mem1[1] - cache1[1] == mem0[1] - cache0[1]                  # blocks
    assert mem1[0] - cache1[0] == mem0[0] - cache0[0]                  # bytes
    assert copies and not [a for a in copies if any(lo <= a < hi for lo, hi in planes)]


@pytest.fixture(scope="module")
def solved(ctx):
    """One inputs.climate(with_spec=True, save_all_profiles=True) run on the premixed table of climate_driver_cases.e2e_case;
    find_strat's entry profile is recorded on the way."""
    case, opa = cd.e2e_case(jdi, px, ctx)
    entry = {}
    real = pc.find_strat

    def find_strat(*a, **k):
        entry["temp"], entry["pressure"] = np.array(a[3], dtype=float), np.array(a[4], dtype=float)
        return real(*a, **k)
    pc.find_strat = find_strat
    try:
        out = case.climate(opa, with_spec=True, save_all_profiles=True, verbose=False)
    finally:
        pc.find_strat = real
    return case, opa, out, entry


def test_climate_end_to_end_satisfies_radiative_convective_equilibrium(ctx, solved):
    """No reference value: what a solution must satisfy, whatever path led to it.  Converged; in every radiative level the
    net flux (recomputed by a fresh get_fluxes call at the returned profile) balances the flux to carry within tolf of
    |tidal[0]|; every convective layer lies on the adiabat of did_grad_cp to 1e-12; no radiative layer is steeper than the
    adiabat of find_strat's entry profile over 0.98; the temperatures lie inside the opacity table's widened range."""
    case, opa, out, entry = solved
    e = cd.E2E
    assert out["converged"] == 1
    temp, pressure, nstr, dtdp = out["temperature"], out["pressure"], list(out["cvz_locs"]), out["dtdp"]
    assert len(temp) == e["nlevel"] and nstr[0] == 0 and 5 <= nstr[1] < nstr[2] == e["nlevel"] - 2
    tmin, tmax = e["temps"].min() * 0.7, e["temps"].max() * 1.3
    assert np.all(temp > tmin) and np.all(temp < tmax)
    fb = out["flux_balance"]
    assert fb["rfacv"] == 0.0 and np.all(fb["tidal"] == -0.56687e-4 * e["teff"] ** 4)
    assert np.array_equal(opa.relative_flux, np.ones(len(e["wno"])))

    case.add_pt(temp, pressure)
    case.premix_atmosphere(opa, verbose=False)
    wed, noed, sp, dis, atm, _ = pc.calculate_atm(case, opa)
    og = pc.Opagrid_Tuple(opa.nwno, opa.delta_wno, opa.wno, opa.ngauss, opa.gauss_wts)
    f = pc.get_fluxes(atm, wed, noed, sp, dis, og, opa.relative_flux, False, True, ctx=ctx)
    net_layer, net, tidal = f[4], f[5], fb["tidal"]
    zones = [(0, nstr[1], nstr[2])] + ([(nstr[3] + 1, nstr[4], nstr[5])] if nstr[3] != 0 else [])
    radiative = [j for lo, hi, _ in zones for j in range(lo, hi + 1)]
    res = np.array([abs(fb["rfaci"] * (net[j] if j == 0 else net_layer[j - 1]) + tidal[j]) for j in radiative]) / abs(tidal[0])
    print("radiative levels %s: max |rfaci F_ir + tidal| / |tidal[0]| = %.2e (bound %.0e)" % (radiative, res.max(), TOLF))
    assert np.all(res < TOLF)

    ad = pc.AdiabatBundle_Tuple(*[case.inputs["climate"][k] for k in ("t_table", "p_table", "grad", "cp")])
    assert np.allclose(dtdp, cd.lapse(temp, pressure), rtol=1e-13, atol=0)
    convective = [j - 1 for _, n_strt, n_bot in zones for j in range(n_strt + 1, n_bot + 2)]
    for layer in convective:
        grad = pc.did_grad_cp(temp[layer], np.sqrt(pressure[layer] * pressure[layer + 1]), ad)[0]
        assert abs(dtdp[layer] - grad) <= 1e-12 * grad, layer
    grad_entry, _ = pc.convec(entry["temp"], entry["pressure"], ad, None)
    for layer in sorted(set(range(e["nlevel"] - 1)) - set(convective)):
        assert dtdp[layer] < grad_entry[layer] / 0.98, layer
    assert len(out["all_profiles"]) % e["nlevel"] == 0 and len(out["all_profiles"]) > 3 * e["nlevel"]
    assert set(out["ptchem_df"].keys()) == {"temperature", "pressure", "H2", "He", "H2O"}


def test_with_spec_is_the_thermal_spectrum_at_the_returned_profile(ctx, solved):
    _, opa, out, _ = solved
    other, _ = cd.e2e_case(jdi, px, ctx)
    other.atmosphere(df={k: np.array(v) for k, v in out["ptchem_df"].items()})
    want = other.spectrum(opa, calculation="thermal", full_output=True)
    got = out["spectrum_output"]
    assert np.array_equal(got["wavenumber"], want["wavenumber"])
    assert np.array_equal(got["thermal"], want["thermal"]) and np.all(got["thermal"] > 0)
