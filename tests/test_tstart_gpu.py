"""The T(P) iteration on the device: climate.get_nets_tbatch (the fused thermal-nets kernel of toon_lvl.hip) against the
level planes of the existing batched path, against tests/golden/climate_fluxes.npz and against itself, and climate.t_start
with the device calls against tests/golden/tstart.npz (what the reference's own t_start did)."""
import numpy as np
import pytest

import tstart_cases as tc
from helpers import rel_err
from picaso_amd import climate as pc
from picaso_amd import resident
from picaso_amd.device import DeviceArray

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    return pc._lib.context()


def _jacobian_profiles(t0, nitem):
    """Profiles as the solver makes them: row k has level k raised by max(1e-4 T, 3 K); row 0 of a single row is t0."""
    t0 = np.asarray(t0, dtype=float)
    rows = [t0 + (np.arange(len(t0)) == k) * max(1e-4 * t0[k], 3.0) for k in range(nitem)]
    return np.stack(rows) if nitem > 1 else t0[None, :].copy()


def _scene(ctx, name):
    """name: a | g1 | holes of climate_fluxes.npz, a3 = `a` tiled 3x along wavenumber (108 columns: a full wave and a
    partial one), a2 = the top layer of `a` alone (2 levels) -> the arguments of get_nets_tbatch, resident planes."""
    base = {"a3": "a", "a2": "a"}.get(name, name)
    g = tc.fixtures()[1]
    (atm, wed, noed, sp, dis, og, _), holes = tc.scene_args(pc, base, g[base + "/plevel"])
    if name == "a3":
        def tile(x):
            return None if x is None else np.ascontiguousarray(np.tile(x, (1, 3, 1)))
        wed, noed = pc.OpacityWEd_Tuple(*[tile(x) for x in wed]), pc.OpacityNoEd_Tuple(*[tile(x) for x in noed])
        og = og._replace(nwno=3 * og.nwno, delta_wno=np.tile(og.delta_wno, 3) * np.repeat([1.0, 0.5, 2.0], og.nwno),
                         wno=np.tile(og.wno, 3))
        sp = sp._replace(surf_reflect=np.tile(sp.surf_reflect, 3))
    if name == "a2":
        def top(x):
            return None if x is None else np.ascontiguousarray(x[:2] if x.shape[0] == atm.nlevel else x[:1])
        wed, noed = pc.OpacityWEd_Tuple(*[top(x) for x in wed]), pc.OpacityNoEd_Tuple(*[top(x) for x in noed])
        atm = atm._replace(nlevel=2, t_level=atm.t_level[:2].copy(), p_level=atm.p_level[:2].copy())

    def up(t):
        return type(t)(*[DeviceArray.from_host(np.ascontiguousarray(x), ctx) if isinstance(x, np.ndarray) else x for x in t])
    wed, noed = up(wed), up(noed)
    if holes:
        holes = dict(holes, hole_OpacityWEd=up(holes["hole_OpacityWEd"]), hole_OpacityNoEd=up(holes["hole_OpacityNoEd"]))
    return (atm, wed, noed, sp, dis, og), holes


def _plane_sums(ctx, temps, args, wed, noed):
    """The existing path's full outputs (picaso_get_thermal_1d_ck_tbatch_dev: flux_minus, flux_plus and their mid-point
    twins, Gauss-weighted and disk-integrated, per wavenumber) summed over wavenumber on the host in extended precision
    -> (net_layer, net), (S_layer, S) with S = sum_w dwno (|plus| + |minus|)."""
    atm, _, _, sp, dis, og = args
    nlevel, nwno, nitem = int(atm.nlevel), int(og.nwno), len(temps)
    pl = pc._planes(wed, noed, ctx, thermal_only=True)
    disk4 = DeviceArray((4, nlevel, nitem * nwno), ctx)
    rs = DeviceArray.from_host(np.zeros(nwno) + np.asarray(sp.surf_reflect, dtype=float), ctx)
    d_wno, d_dw = DeviceArray.from_host(og.wno, ctx), DeviceArray.from_host(og.delta_wno, ctx)
    resident.thermal_1d_ck_tbatch(ctx, nlevel, d_wno, nwno, int(og.ngauss), int(dis.ng), int(dis.nt), temps, pl["dtau_og"],
                                  pl["w0_no_raman"], pl["cosb_og"], atm.p_level, dis.ubar1, rs, 0, og.gauss_wts, dis.gweight,
                                  dis.tweight, disk4, dwno=d_dw, calc_type=1)
    fm, fp, fmm, fpm = disk4.to_host().reshape(4, nlevel, nitem, nwno).astype(np.longdouble)
    dw = np.asarray(og.delta_wno, dtype=np.longdouble)

    def sums(plus, minus):
        return (((plus - minus) * dw).sum(axis=2).T.astype(float), ((np.abs(plus) + np.abs(minus)) * dw).sum(axis=2).T.astype(float))
    (nl, sl), (n, s) = sums(fpm, fmm), sums(fp, fm)
    return (nl, n), (sl, s)


@pytest.mark.parametrize("name", ["a", "g1", "holes", "a3", "a2"])
def test_nets_match_the_sums_of_the_level_planes(ctx, name):
    """Every net within (N + 8) 2^-52 S of the host sums of the existing path's planes, N = nang ngauss nwno terms per
    row and S = sum |weights| (|flux_plus| + |flux_minus|) of that row: the bound of re-ordering the sums and
    re-associating the weights, given that every per-column flux carries the existing kernel's bits.  The excess over the
    bound is printed before it is asserted."""
    args, holes = _scene(ctx, name)
    atm, wed, noed, sp, dis, og = args
    nlevel = int(atm.nlevel)
    N = int(dis.ng) * int(dis.nt) * int(og.ngauss) * int(og.nwno)
    for nitem in (1, 3, nlevel):
        temps = _jacobian_profiles(atm.t_level, min(nitem, nlevel))
        if len(temps) < nitem:                                    # the 2-level scene: three profiles all the same
            temps = np.concatenate([temps, temps * 1.01])[:nitem]
        got = pc.get_nets_tbatch(temps, *args, ctx=ctx, **holes)
        want, S = _plane_sums(ctx, temps, args, wed, noed)
        if holes:
            f = holes["fhole"]
            wc, Sc = _plane_sums(ctx, temps, args, holes["hole_OpacityWEd"], holes["hole_OpacityNoEd"])
            want = [(1.0 - f) * a + f * b for a, b in zip(want, wc)]
            S = [(1.0 - f) * a + f * b for a, b in zip(S, Sc)]
        for g_, w_, s_, what in zip(got, want, S, ("net_layer", "net")):
            assert g_.shape == (nitem, nlevel)
            bound = (N + 8) * ULP * s_
            worst = float(np.max(np.abs(g_ - w_) / np.where(bound > 0, bound, 1.0)))
            print("%s nitem=%d %s: worst |diff| / bound = %.3f" % (name, nitem, what, worst))
            assert np.all(np.abs(g_ - w_) <= bound), (name, nitem, what, worst)
    assert np.array_equal(got[0][:, -1], np.zeros(nitem))         # no mid-point below the last level


@pytest.mark.parametrize("ng,nt", [(1, 1), (2, 2), (3, 2), (6, 1), (7, 1), (8, 1), (3, 3), (5, 2)])
def test_nets_match_for_every_compiled_angle_count(ctx, ng, nt):
    """The fused kernel is compiled once per angle count, and with nt > 1 it takes tweight[k % nt], the (g, t) angle order
    and compress_thermal's 1 / (2 pi): 1, 4, 6, 7, 8, 9 and 10 angles (5 is every other test; 2 and 3 have no geometry)
    against the plane path under the same bound, on the 7-wavenumber scene (the tightest bound) and on the scene with
    doubled bin widths in its third tile, whose thin top layers amplify a differently rounded product the most."""
    from picaso_amd import disco
    if nt == 1 and ng >= 5:
        g, gw, t, tw = disco.get_angles_1d(ng)
    else:
        g, gw, t, tw = disco.get_angles_3d(ng, nt)
    u0, u1, _, _, _ = disco.compute_disco(ng, nt, g, t, 0.0)
    assert ng * nt <= resident.thermal_nets_max_angles()
    for name in ("g1", "a3"):
        (atm, wed, noed, sp, _, og), _ = _scene(ctx, name)
        args = (atm, wed, noed, sp, pc.Disco_Tuple(ng, nt, gw, tw, u0, u1, 1.0), og)
        temps = _jacobian_profiles(atm.t_level, 3)
        got = pc.get_nets_tbatch(temps, *args, ctx=ctx)
        want, S = _plane_sums(ctx, temps, args, wed, noed)
        N = ng * nt * int(og.ngauss) * int(og.nwno)
        for g_, w_, s_, what in zip(got, want, S, ("net_layer", "net")):
            bound = (N + 8) * ULP * s_
            worst = float(np.max(np.abs(g_ - w_) / np.where(bound > 0, bound, 1.0)))
            print("%s %dx%d %s: worst |diff| / bound = %.3f" % (name, ng, nt, what, worst))
            assert np.all(np.abs(g_ - w_) <= bound), (name, ng, nt, what, worst)


@pytest.mark.parametrize("c", ["a", "holes", "g1"])
def test_nets_meet_the_reference_fixture(ctx, c):
    """tests/test_climate_fluxes.py's check of the IR nets against the reference's own get_fluxes outputs; for `holes`
    the blended nets."""
    g = tc.fixtures()[1]
    args, holes = _scene(ctx, c)
    net_layer, net = pc.get_nets_tbatch(np.asarray(args[0].t_level)[None, :], *args, ctx=ctx, **holes)
    for got, name in ((net_layer[0], "flux_net_ir_layer"), (net[0], "flux_net_ir")):
        want = g["%s/out/%s" % (c, name)]
        assert rel_err(got, want, 1e-4 * np.abs(want).max()) < 2e-8, (c, name)


@pytest.mark.parametrize("name", ["a", "holes", "a3"])
def test_nets_are_deterministic_and_independent_of_the_batch(ctx, name):
    """Two calls return equal bits; row k of an nlevel-profile call equals the one-profile call on profile k."""
    args, holes = _scene(ctx, name)
    temps = _jacobian_profiles(args[0].t_level, int(args[0].nlevel))
    first = pc.get_nets_tbatch(temps, *args, ctx=ctx, **holes)
    again = pc.get_nets_tbatch(temps, *args, ctx=ctx, **holes)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for k in range(len(temps)):
        alone = pc.get_nets_tbatch(temps[k:k + 1], *args, ctx=ctx, **holes)
        assert all(np.array_equal(a[0], b[k]) for a, b in zip(alone, first)), k
    with pytest.raises(Exception, match="nlevel"):
        pc.get_nets_tbatch(temps[:, :-1], *args, ctx=ctx, **holes)


def test_nets_beyond_the_compiled_angle_count_use_the_plane_path(ctx):
    """More disk angles than the fused kernel carries in registers: the documented route through get_fluxes_tbatch."""
    from picaso_amd import disco
    args, _ = _scene(ctx, "g1")
    atm, wed, noed, sp, dis, og = args
    ng, nt = 7, 2
    assert ng * nt > resident.thermal_nets_max_angles()
    g, gw, t, tw = disco.get_angles_3d(ng, nt)
    u0, u1, _, _, _ = disco.compute_disco(ng, nt, g, t, 0.0)
    many = pc.Disco_Tuple(ng, nt, gw, tw, u0, u1, 1.0)
    temps = _jacobian_profiles(atm.t_level, 3)
    got = pc.get_nets_tbatch(temps, atm, wed, noed, sp, many, og, ctx=ctx)
    want = pc.get_fluxes_tbatch(temps, atm, wed, noed, sp, many, og, ctx=ctx, nets_only=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(pc._lib.PicasoHipError, match="angles"):
        out = DeviceArray((2, 3, int(atm.nlevel)), ctx)
        pl = pc._planes(wed, noed, ctx, thermal_only=True)
        v = DeviceArray.from_host(np.asarray(og.wno, dtype=float), ctx)
        resident.thermal_nets_tbatch(ctx, int(atm.nlevel), v, int(og.nwno), int(og.ngauss), ng, nt, temps, pl["dtau_og"],
                                     pl["w0_no_raman"], pl["cosb_og"], atm.p_level, u1, v, 0, og.gauss_wts, gw, tw, v,
                                     out.row_block(0), out.row_block(1))


def _device_fluxes(ctx, seen):
    def single(atm, *a, **k):
        seen.append(np.array(atm.t_level, dtype=float))
        return pc.get_fluxes(atm, *a, ctx=ctx, **k)

    def batched(temps, *a, **k):
        seen.extend(np.array(temps, dtype=float))
        return pc.get_nets_tbatch(temps, *a, ctx=ctx, **k)
    return single, batched


@pytest.mark.parametrize("case,call", tc.case_calls())
def test_t_start_on_the_device_follows_the_reference(ctx, case, call):
    """The reference's number of evaluations (plus the closing thermal call), the final temperature within the fixture's
    tol_temp, and flux_plus_ir[0, :] within test_climate_fluxes' level-flux metric at 2e-4 of the oracle's get_fluxes at
    the temperature t_start itself returned."""
    from oracle import climate_oracle as co
    ts = tc.fixtures()[0]
    tag = "%s/%d/" % (case, call)

    def up(x):
        return DeviceArray.from_host(np.ascontiguousarray(x), ctx)
    seen = []
    out, atm, _ = tc.run(pc, case, call, up=up, _fluxes=_device_fluxes(ctx, seen))
    temp, plus_top = out[0], out[5]
    want = ts[tag + "profiles"]
    at_root = len(want) == 1
    assert len(seen) == len(want) + (0 if at_root else 1), (len(seen), len(want))
    assert np.array_equal(atm.t_level, ts[tag + "t_in"])
    gap = float(np.max(np.abs(temp - ts[tag + "temp"]) / ts[tag + "temp"]))
    print("%s: max |T - T_ref| / T_ref = %.2e, tol_temp = %.2e" % (tag, gap, float(ts[tag + "tol_temp"])))
    assert gap <= float(ts[tag + "tol_temp"])
    (_, wed, noed, sp, dis, og, f0pi), holes = tc.scene_args(pc, str(ts[case + "/scene"]), ts[case + "/plevel"], t_level=temp)
    ref = co.get_fluxes(atm._replace(t_level=temp), wed, noed, sp, dis, og, f0pi, False, True, **holes)
    scale = np.maximum(np.abs(ref[6]).max(axis=0), np.abs(ref[7]).max(axis=0))
    scale = np.where(scale == 0, 1.0, scale)
    assert np.max(np.abs(plus_top - ref[6][0]) / scale) < 2e-4


def test_t_start_is_deterministic_on_its_default_path(ctx):
    """Two calls without injected callables (get_fluxes and get_nets_tbatch on the process's context) return equal bits,
    and the same bits as the instrumented run of the test above."""
    def up(x):
        return DeviceArray.from_host(np.ascontiguousarray(x), ctx)
    first, atm, _ = tc.run(pc, "one_noegp", 1, up=up)
    again, _, _ = tc.run(pc, "one_noegp", 1, up=up)
    wrapped, _, _ = tc.run(pc, "one_noegp", 1, up=up, _fluxes=_device_fluxes(ctx, []))
    for a, b, c in zip(first, again, wrapped):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert first[0] is not atm.t_level
