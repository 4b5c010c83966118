"""The T(P) iteration on the host: picaso_amd.climate.t_start and its helpers against tests/golden/tstart.npz, what the
reference's own climate.t_start, did_grad_cp, convec, locate and mat_sol did (tests/golden/make_tstart.py).  The flux
calls are oracle.climate_oracle.get_fluxes through t_start's `_fluxes` injection, so nothing here needs a GPU."""
import numpy as np
import pytest

import tstart_cases as tc
from picaso_amd import climate as pc

ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def ts():
    return tc.fixtures()[0]


def test_adiabat_helpers_match_the_reference(ts):
    """locate exactly; did_grad_cp (scalar and array call) and convec within 4 ulp: the same arithmetic, only log10 and
    10**x may differ in their last bits.  The samples include points off every edge of the table."""
    ad = tc.adiabat(pc)
    t, p = ts["adiabat/sample_t"], ts["adiabat/sample_p"]
    assert (np.log10(t) < ad.t_table[0]).any() and (np.log10(t) > ad.t_table[-1]).any()
    assert (np.log10(p) < ad.p_table[0]).any() and (np.log10(p) > ad.p_table[-1]).any()
    assert np.array_equal([pc.locate(ad.t_table, x) for x in np.log10(t)], ts["adiabat/locate_t"])
    assert np.array_equal(pc.locate(ad.p_table, np.log10(p)), ts["adiabat/locate_p"])
    grad, cp = pc.did_grad_cp(t, p, ad)
    one = np.array([pc.did_grad_cp(a, b, ad) for a, b in zip(t, p)])
    for got in ((grad, cp), (one[:, 0], one[:, 1])):
        assert np.all(np.abs(got[0] - ts["adiabat/sample_grad"]) <= 4 * ULP * np.abs(ts["adiabat/sample_grad"]))
        assert np.all(np.abs(got[1] - ts["adiabat/sample_cp"]) <= 4 * ULP * np.abs(ts["adiabat/sample_cp"]))
    assert isinstance(pc.did_grad_cp(300.0, 1.0, ad)[0], float)
    g, c = pc.convec(ts["adiabat/convec_t"], ts["adiabat/convec_p"], ad, None)
    assert np.all(np.abs(g - ts["adiabat/convec_grad"]) <= 4 * ULP * np.abs(ts["adiabat/convec_grad"]))
    assert np.all(np.abs(c - ts["adiabat/convec_cp"]) <= 4 * ULP * np.abs(ts["adiabat/convec_cp"]))
    with pytest.raises(NotImplementedError):
        pc.convec(ts["adiabat/convec_t"], ts["adiabat/convec_p"], ad, None, moist=True)


def test_mat_sol_on_the_recorded_systems(ts):
    """Every (A, b) the reference's t_start handed to its mat_sol: the recorded p within 1e-11 max|p|, and the residual
    |A p - b| <= 1e-10 (|A| |p| + |b|).  The matrix sits in the corner of an nlevel x nlevel array, as t_start passes it."""
    n_sys = 0
    for c, k in tc.case_calls():
        tag = "%s/%d/" % (c, k)
        if tag + "mat_A" not in ts:
            continue
        for A, b, p in zip(ts[tag + "mat_A"], ts[tag + "mat_b"], ts[tag + "mat_p"]):
            n = len(b)
            assert n in (10, 12, 13, 15)                             # the unknowns of the four zone vectors
            a, rhs = np.zeros((21, 21)), np.zeros(21)
            a[:n, :n], rhs[:n] = A, b
            a_out, got = pc.mat_sol(a, 21, n, rhs)
            assert a_out is a and got is rhs
            assert np.max(np.abs(got[:n] - p)) <= 1e-11 * np.abs(p).max(), tag
            assert np.all(np.abs(A @ got[:n] - b) <= 1e-10 * (np.abs(A) @ np.abs(got[:n]) + np.abs(b))), tag
            n_sys += 1
    assert n_sys > 50


def test_mat_sol_pivot_rule_and_limits():
    """Tied scaled pivots: the LAST tied row wins (dum >= aamax), which the solution cannot show but the factors do;
    a singular row raises; 128 levels are accepted."""
    a = np.array([[2.0, 1.0, 0.0], [4.0, 1.0, 2.0], [1.0, 0.5, 0.25]])      # column 0 scaled: 1, 1, 1 -> row 2 is the pivot
    lu, x = pc.mat_sol(a.copy(), 3, 3, np.array([1.0, 2.0, 3.0]))
    assert lu[0, 0] == 1.0 and np.array_equal(lu[0], [1.0, 0.5, 0.25])
    assert np.allclose(a @ x, [1.0, 2.0, 3.0], rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match="singular"):
        pc.mat_sol(np.array([[0.0, 0.0], [1.0, 2.0]]), 2, 2, np.ones(2))
    rng = np.random.default_rng(0)
    big = rng.normal(size=(128, 128)) + 20 * np.eye(128)
    rhs = rng.normal(size=128)
    _, x = pc.mat_sol(big.copy(), 128, 128, rhs.copy())
    assert np.all(np.abs(big @ x - rhs) <= 1e-10 * (np.abs(big) @ np.abs(x) + np.abs(rhs)))
    with pytest.raises(ValueError):
        pc.mat_sol(np.eye(129), 129, 129, np.ones(129))


def test_check_convergence_and_zone_growth():
    n = 3
    f_vec, g, dflux = np.array([1e-3, -2e-3, 1e-3, 9.0]), np.ones(4), np.full(4, 1e-7)
    t_old = np.array([100.0, 200.0, 300.0, 400.0])
    assert pc.check_convergence(f_vec, n, 5e-3, True, 1.0, dflux, 1e-5, t_old, t_old, g, 5e-3) == (2, False)
    f_vec[1] = 1.0
    assert pc.check_convergence(f_vec, n, 5e-3, True, 1.0, dflux, 1e-5, t_old, t_old, g, 5e-3) == (2, True)
    assert pc.check_convergence(f_vec, n, 5e-3, True, 1.0, dflux * 1e4, 1e-5, t_old, t_old, g, 5e-3) == (2, False)
    assert pc.check_convergence(f_vec, n, 5e-3, False, 1.0, dflux, 1e-5, t_old * 1.001, t_old, g, 5e-3) == (2, False)
    t_new = t_old * np.array([1.0, 1.01, 1.0, 1.0])
    assert pc.check_convergence(f_vec, n, 5e-3, False, 1.0, dflux, 1e-5, t_new, t_old, g, 5e-3) == (1, False)
    t_new = t_old * np.array([1.0, 1.0, 1.0, 2.0])                       # beyond n_total: not looked at
    assert pc.check_convergence(f_vec, n, 5e-3, False, 1.0, dflux, 1e-5, t_new, t_old, g, 5e-3) == (2, False)
    assert list(pc.growup(1, np.array([0, 12, 19, 0, 0, 0]), 2)) == [0, 10, 19, 0, 0, 0]
    assert list(pc.growup(2, np.array([0, 6, 9, 9, 14, 19]), 1)) == [0, 6, 9, 9, 13, 19]
    assert list(pc.growdown(1, np.array([0, 6, 9, 9, 14, 19]), 1)) == [0, 6, 10, 10, 14, 19]


def test_opagrid_tuple_keeps_its_five_argument_form():
    og = pc.Opagrid_Tuple(3, np.ones(3), np.arange(3.0), 1, np.ones(1))
    assert og.tmin == -np.inf and og.tmax == np.inf and og._fields[-2:] == ("tmin", "tmax")
    assert pc.Opagrid_Tuple(3, None, None, 1, None, 75.0, 4000.0).tmax == 4000.0


def _oracle_fluxes(seen):
    from oracle import climate_oracle as co

    def single(atm, *a, **k):
        seen.append(np.array(atm.t_level, dtype=float))
        return co.get_fluxes(atm, *a, **k)
    return (single, None)


@pytest.mark.parametrize("case,call", tc.case_calls())
def test_t_start_over_the_oracle_follows_the_reference(ts, case, call):
    """The whole iteration with the oracle's get_fluxes: the reference's number of evaluations (plus the one thermal call
    at the accepted profile, which a call that starts at a root does not need), the first Jacobian's profiles, the final
    temperature within the fixture's tol_temp, dtdp of that temperature, the saved profiles; t_level left alone."""
    tag = "%s/%d/" % (case, call)
    seen = []
    out, atm, _ = tc.run(pc, case, call, _fluxes=_oracle_fluxes(seen))
    temp, dtdp, all_profiles, fourth, net_v, plus_top = out
    want = ts[tag + "profiles"]
    at_root = len(want) == 1
    assert len(seen) == len(want) + (0 if at_root else 1), (len(seen), len(want))
    assert np.array_equal(atm.t_level, ts[tag + "t_in"]) and np.array_equal(seen[0], atm.t_level)
    if not at_root:
        n_total = ts[tag + "mat_b"].shape[1]
        got = np.array(seen[1:1 + n_total])
        assert np.max(np.abs(got - want[1:1 + n_total]) / want[1:1 + n_total]) <= 1e-13
        assert np.array_equal(seen[-1], temp)
    tol = float(ts[tag + "tol_temp"])
    assert np.max(np.abs(temp - ts[tag + "temp"]) / ts[tag + "temp"]) <= tol
    p = ts[case + "/plevel"]
    lapse = (np.log(temp[:-1]) - np.log(temp[1:])) / (np.log(p[:-1]) - np.log(p[1:]))
    assert np.allclose(dtdp, lapse, rtol=1e-14, atol=0)
    assert all_profiles.shape == ts[tag + "all_profiles"].shape
    assert np.allclose(all_profiles, ts[tag + "all_profiles"], rtol=50 * tol, atol=0)
    assert np.array_equal(all_profiles[:len(temp)], ts[tag + "t_in"]) or at_root
    # the fluxes are those of the returned profile: within the flux response to tol_temp of the reference's
    scale = np.abs(ts[tag + "flux_fourth"]).max()
    assert np.max(np.abs(fourth - ts[tag + "flux_fourth"])) <= max(1e-8, 100 * tol) * scale
    assert np.max(np.abs(net_v - ts[tag + "flux_net_v"])) <= 1e-8 * np.abs(ts[tag + "flux_net_v"]).max()
    assert np.max(np.abs(plus_top - ts[tag + "flux_plus_top"])) <= max(1e-8, 100 * tol) * np.abs(ts[tag + "flux_plus_top"]).max()


def test_root_and_clamp_behave_as_recorded(ts):
    last = int(ts["root/ncall"]) - 1
    assert ts["root/%d/profiles" % last].shape[0] == 1 and np.array_equal(ts["root/%d/temp" % last], ts["root/%d/t_in" % last])
    seen = []
    out, atm, _ = tc.run(pc, "root", last, _fluxes=_oracle_fluxes(seen))
    assert len(seen) == 1 and np.array_equal(out[0], atm.t_level) and out[0] is not atm.t_level
    assert out[2].size == 0                                            # no iteration, no saved profile
    tmax = float(ts["clamp/tmax"])
    assert tmax < ts["clamp/0/t_in"].max()
    seen = []
    out, _, _ = tc.run(pc, "clamp", 0, _fluxes=_oracle_fluxes(seen))
    hit = [np.flatnonzero(p == tmax - 0.1) for p in seen[1:]]
    ref_hit = [np.flatnonzero(p == tmax - 0.1) for p in ts["clamp/0/profiles"][1:]]
    assert any(len(h) for h in ref_hit)
    assert all(np.array_equal(a, b) for a, b in zip(hit, ref_hit))
    assert out[0].max() == tmax - 0.1 == ts["clamp/0/temp"].max()


def _linear_fluxes(t_star, k_lin, tidal0, seen):
    """A flux function that is all but linear in the level temperatures, so that one Newton step lands next to the root:
    every residual is k_lin d + 1e3 d^2, d = T - t_star at its own unknown level (the step from d = 1 leaves ~4e3, far
    above the absolute tolf and far below 5e-5 |tidal|), and flux_plus_ir[0, :] is T[0] of the profile it was evaluated at."""
    def single(atm, wed, noed, sp, dis, og, f0pi, reflected, thermal, **kw):
        t = np.array(atm.t_level, dtype=float)
        seen.append(t)
        n = len(t)
        d = t - t_star
        net = k_lin * d + 1e3 * d ** 2 - tidal0                    # the level nets; only level 0 is a residual
        net_layer = np.append(net[1:], 0.0)                        # mid-point j is the residual of level j + 1
        plus = np.tile(t[:, None], (1, og.nwno))
        zeros = np.zeros((dis.ng, dis.nt, n))
        return zeros, zeros, None, None, net_layer, net, plus, np.zeros_like(plus)
    return single, None


def test_root_exit_after_an_iteration_returns_the_fluxes_of_the_returned_profile(ts):
    """The "already at a root" test runs at the top of every iteration.  When it fires after a step (the step moved T by
    more than tolx and left a residual below 5e-5 |tidal| but above the absolute tolf), the line-search trials have given
    nets only, so flux_plus_ir[0, :] must come from an evaluation of the returned profile, not of the starting one."""
    (atm, wed, noed, sp, dis, og, f0pi), _ = tc.scene_args(pc, "a", ts["one/plevel"], 10.0, 1.0e5)
    t_star = np.array(atm.t_level, dtype=float)
    start = t_star.copy()
    start[:13] += 1.0                                              # the unknowns of nstr; below the step cap (~6 K in norm)
    seen = []
    conv = pc.convergence_criteriaT(15, 7, 5.0, 5.0, 7.0)
    tidal = np.full(len(t_star), 1e14)
    out = pc.t_start(1, [0, 12, 19, 0, 0, 0], conv, 1.0, 0.0, tidal, atm._replace(t_level=start), wed, noed, sp, dis, og,
                     tc.adiabat(pc), f0pi, 0, np.zeros(0), verbose=0, egp_stepmax=True,
                     _fluxes=_linear_fluxes(t_star, 1e12, 1e14, seen))
    temp, plus_top = out[0], out[5]
    # first evaluation, 13 Jacobian profiles, one trial that lands on the root (flag 1: T moved by 1/150 > tolx), then the
    # root exit of iteration 1 and its one evaluation of the returned profile
    assert len(seen) == 1 + 13 + 1 + 1
    assert np.allclose(temp[:13], t_star[:13], rtol=1e-9, atol=0) and abs(start[0] - temp[0]) > 0.9
    assert np.array_equal(seen[-1], temp)
    assert np.array_equal(plus_top, np.full(og.nwno, temp[0]))
    d = temp - t_star
    assert np.array_equal(out[3], 1e12 * d + 1e3 * d ** 2 - 1e14)  # flux_net_ir of the returned profile too
    assert 5e-3 < np.abs(out[3][0] + 1e14) < 5e-5 * 1e14           # not converged by tolf, a root by the relative test


def test_moist_raises_and_arguments_are_checked(ts):
    with pytest.raises(NotImplementedError):
        tc.run(pc, "one", 0, _fluxes=_oracle_fluxes([]), moist=True)
    with pytest.raises(NotImplementedError):
        pc.t_start(1, [0, 1, 2, 0, 0, 0], None, 1.0, 0.0, None, None, None, None, None, None, None, None, None, 0, None,
                   moist=True)


def test_load_adiabat_reads_the_reference_layout(ts, tmp_path, monkeypatch):
    import json
    ad = tc.adiabat(pc)
    d = tmp_path / "climate_INPUTS"
    d.mkdir()
    (d / "specific_heat_p_adiabat_grad.json").write_text(json.dumps(dict(
        temperature=ad.t_table.tolist(), pressure=ad.p_table.tolist(), adiabat_grad=ad.grad.tolist(),
        specific_heat=ad.cp.tolist())))
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    got = pc.load_adiabat()
    assert all(np.array_equal(a, b) for a, b in zip(got, ad)) and got.grad.shape == (53, 26)
    monkeypatch.delenv("picaso_refdata")
    with pytest.raises(Exception, match="picaso_refdata"):
        pc.load_adiabat()
