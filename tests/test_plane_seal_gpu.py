"""Seals of resident reflected plane sets (csrc/planeseal.hip, the launcher in csrc/api.hip).

``upload_scene`` verifies ONCE that ``tau`` / ``tau_og`` are the running sums of ``dtau`` / ``dtau_og`` from +0.0 and that
``gcos2`` is ``0.5 ftau_ray``; launches on a sealed set that would take a kernel which knows the absent-planes pattern at
compile time (five angles, zero phase: ``k_reflected_coop<true, 3>``, ``k_reflected_toa<5, false, true, true, false, 3>``
and its batched form) are then run as if the three planes had been left out.  What is checked here: which sets seal,
which launches use a seal (``picaso_reflected_seal_stat``), that a seal dies with its bytes, and that every launch,
substituted or not, returns the bits of the same call with ``PICASO_AMD_REFL_ALL_PLANES=1``.

The scene is ``make_scene(6, 200)``: seven levels, four waves of which the last is partial, a cloud in layers 3-4.  At
200 columns the fused launch would by itself spread the angles over waves or take the one-wave-per-SIMD form, neither of
which substitutes; ``FUSED`` pins the shape the 1e5-column launch has (all angles in one lane, two waves per SIMD)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)
NLAYER, NWNO = 6, 200
COOP = {}
FUSED = {"PICASO_AMD_REFL_COOP_COLS": "0", "PICASO_AMD_ANGLE_GROUP": "0", "PICASO_AMD_REFL_NO_BIG": "1"}
KNOBS = ("PICASO_AMD_REFL_ALL_PLANES", "PICASO_AMD_REFL_GENERIC", "PICASO_AMD_REFL_NO_COOP", "PICASO_AMD_MAX_ANGLES") + \
    tuple(FUSED)


def _scene(seed=21):
    from picaso_amd import synthetic as syn
    sc = syn.make_scene(NLAYER, NWNO, seed=seed)
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    sc["F0PI"] = np.linspace(0.9, 1.1, NWNO)
    sc["surf_reflect"] = np.full(NWNO, 0.15)
    assert sc["ftau_cld"][3:5].min() > 0 and sc["ftau_cld"][:3].max() == 0        # the cloud is inside
    return sc


def _keys():
    from picaso_amd import resident
    return resident.REFLECTED_PLANES + ("F0PI", "surf_reflect")


def _geometry(ng=5):
    from picaso_amd import disco
    g, gw, t, tw = disco.get_angles_1d(5)
    u0, u1, _, _, _ = disco.compute_disco(5, 1, g, t, 0.0)
    return u0[:ng], u1[:ng], gw[:ng], tw          # fewer than five: the first ones of the five-point rule


def _solve(ctx, d, ng=5, single_phase=3, lvl=False):
    """One ``picaso_get_reflected_1d_dev`` call on the resident set ``d``; returns every output as host arrays."""
    from picaso_amd import _lib, device, resident
    nwno = d["tau"].shape[1]
    u0, u1, gw, tw = _geometry(ng)
    x, alb = device.DeviceArray((ng, 1, nwno), ctx), device.DeviceArray((nwno,), ctx)
    lv = [device.DeviceArray((ng, NLAYER + 1, nwno), ctx) for _ in range(4)] if lvl else [None] * 4
    _lib.check(_lib.load().picaso_get_reflected_1d_dev(
        ctx, NLAYER + 1, nwno, nwno, ng, 1, *[_lib.addr(d[k]) for k in resident.REFLECTED_PLANES],
        _lib.addr(d["surf_reflect"]), _lib.ptr(_lib.f64(u0, (ng, 1))), _lib.ptr(_lib.f64(u1, (ng, 1))), 1.0,
        _lib.addr(d["F0PI"]), single_phase, 0, *TTHG, 1, 1 if lvl else 0, 0, 0.0, _lib.addr(x),
        *[_lib.addr(a) for a in lv], _lib.ptr(_lib.f64(gw)), _lib.ptr(_lib.f64(tw)), _lib.addr(alb)), ctx)
    return [x.to_host(), alb.to_host()] + [a.to_host() for a in lv if a is not None]


def _solve_batch(ctx, sets):
    from picaso_amd import device, resident
    u0, u1, gw, tw = _geometry(5)
    xs = [device.DeviceArray((5, 1, NWNO), ctx) for _ in sets]
    albs = [device.DeviceArray((NWNO,), ctx) for _ in sets]
    resident.reflected_1d_batch(ctx, NLAYER + 1, NWNO, 5, 1, sets, [s["surf_reflect"] for s in sets], u0, u1, 1.0,
                                [s["F0PI"] for s in sets], 3, 0, *TTHG, xs, gweight=gw, tweight=tw, albedo=albs)
    return [a.to_host() for a in xs + albs]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def _ab(monkeypatch, ctx, env, run):
    """``run()`` with the seals in force and again with ``PICASO_AMD_REFL_ALL_PLANES=1``: (hits of the first run, its
    outputs, the all-planes outputs)."""
    from picaso_amd import resident
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h0 = resident.reflected_seal_stat(ctx)[1]
    out = run()
    hits = resident.reflected_seal_stat(ctx)[1] - h0
    monkeypatch.setenv("PICASO_AMD_REFL_ALL_PLANES", "1")
    ref = run()
    assert resident.reflected_seal_stat(ctx)[1] == h0 + hits, "the all-planes run must not use a seal"
    monkeypatch.delenv("PICASO_AMD_REFL_ALL_PLANES")
    return hits, out, ref


def _upload(sc, ctx, lo=None, hi=None):
    """Upload without sealing, then seal by hand to see the flags: (planes, flags)."""
    from picaso_amd import resident
    d = resident.upload_scene(sc, _keys(), lo, hi, ctx=ctx, seal=False)
    nwno = d["tau"].shape[1]
    return d, resident.seal_reflected_planes(ctx, NLAYER + 1, nwno, d)


@pytest.fixture
def ctx():
    from picaso_amd import _lib
    return _lib.context()


# ------------------------------------------------------------------------------------------------------------------------
# 1. seal accepted
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [COOP, FUSED], ids=["coop", "fused"])
def test_sealed_set_is_used_and_gives_the_same_bits(monkeypatch, ctx, env):
    from picaso_amd import resident
    sc = _scene()
    n0 = resident.reflected_seal_stat(ctx)[0]
    d = resident.upload_scene(sc, _keys(), ctx=ctx)                  # seals by itself
    assert resident.reflected_seal_stat(ctx)[0] == n0 + 1
    assert resident.seal_reflected_planes(ctx, NLAYER + 1, NWNO, d) == 7      # sealing again: same flags, still one seal
    assert resident.reflected_seal_stat(ctx)[0] == n0 + 1
    hits, out, ref = _ab(monkeypatch, ctx, env, lambda: _solve(ctx, d) + _solve(ctx, d))
    assert hits == 2                                                  # one per launch
    assert _same(out, ref)
    assert np.isfinite(out[1]).all() and out[1].max() > 0


def test_batch_of_sealed_sets(monkeypatch, ctx):
    from picaso_amd import resident
    sets = [resident.upload_scene(_scene(seed), _keys(), ctx=ctx) for seed in (21, 22)]
    hits, out, ref = _ab(monkeypatch, ctx, FUSED, lambda: _solve_batch(ctx, sets))
    assert hits == 1
    assert _same(out, ref)
    assert _same([out[0], out[2]], _solve(ctx, sets[0]))              # and the member's own launch


# ------------------------------------------------------------------------------------------------------------------------
# 2. seal refused (or, the last case, not)
# ------------------------------------------------------------------------------------------------------------------------
def _ulp(sc, key, i, j):
    sc[key][i, j] = np.nextafter(sc[key][i, j], np.inf)


def _tau_from(sc, start):
    t = np.empty(NLAYER + 1)
    t[0] = start
    for i in range(NLAYER):
        t[i + 1] = t[i] + sc["dtau"][i, 5]
    sc["tau"][:, 5] = t


def _nan(sc):
    sc["dtau"][4, 64] = np.nan


def _last_tau_og(sc):
    sc["tau_og"][NLAYER] *= 3.0


REFUSALS = {
    # name: (edit of the host scene, flags the seal must return)
    "tau_one_ulp": (lambda sc: _ulp(sc, "tau", 3, 77), 7 & ~1),
    "tau_og_one_ulp": (lambda sc: _ulp(sc, "tau_og", 2, 0), 7 & ~2),
    "tau_starts_at_1e-3": (lambda sc: _tau_from(sc, 1e-3), 7 & ~1),
    "tau_starts_at_minus_zero": (lambda sc: _tau_from(sc, -0.0), 7 & ~1),
    "gcos2_perturbed": (lambda sc: _ulp(sc, "gcos2", 1, 199), 7 & ~4),
    "nan_in_dtau": (_nan, 7 & ~1),
    "tau_og_last_level": (_last_tau_og, 7),              # never read by the solver: still seals
}


@pytest.mark.parametrize("env", [COOP, FUSED], ids=["coop", "fused"])
@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_set_that_is_not_derivable_keeps_its_planes(monkeypatch, ctx, name, env):
    from picaso_amd import resident
    edit, want = REFUSALS[name]
    sc = _scene()
    edit(sc)
    n0 = resident.reflected_seal_stat(ctx)[0]
    d, flags = _upload(sc, ctx)
    assert flags == want
    assert resident.reflected_seal_stat(ctx)[0] == n0 + (1 if want == 7 else 0)
    hits, out, ref = _ab(monkeypatch, ctx, env, lambda: _solve(ctx, d))
    assert hits == (1 if want == 7 else 0)
    assert _same(out, ref)
    if name == "nan_in_dtau":
        assert np.isnan(out[1][64]) and np.isfinite(np.delete(out[1], 64)).all()


# ------------------------------------------------------------------------------------------------------------------------
# 3. stale seals
# ------------------------------------------------------------------------------------------------------------------------
def test_a_copy_into_a_sealed_plane_unseals_it(monkeypatch, ctx):
    from picaso_amd import _lib, resident
    sc = _scene()
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    n1 = resident.reflected_seal_stat(ctx)[0]
    hits, before, _ = _ab(monkeypatch, ctx, COOP, lambda: _solve(ctx, d))
    assert hits == 1
    tau2 = np.ascontiguousarray(sc["tau"] * 1.5)
    _lib.check(_lib.load().picaso_memcpy_h2d(ctx, d["tau"].addr, _lib.ptr(tau2), tau2.nbytes), ctx)
    assert resident.reflected_seal_stat(ctx)[0] == n1 - 1
    hits, out, ref = _ab(monkeypatch, ctx, COOP, lambda: _solve(ctx, d))
    assert hits == 0
    assert _same(out, ref)
    assert not np.array_equal(out[1], before[1])          # the new values were honoured
    # the same planes uploaded afresh (never sealed): the same bits
    sc["tau"] = tau2
    fresh = resident.upload_scene(sc, _keys(), ctx=ctx, seal=False)
    assert _same(out, _solve(ctx, fresh))


def test_a_copy_next_to_a_sealed_plane_leaves_the_seal(ctx):
    from picaso_amd import _lib, device, resident
    d = resident.upload_scene(_scene(), _keys(), ctx=ctx)
    n1 = resident.reflected_seal_stat(ctx)[0]
    other = device.DeviceArray.from_host(np.zeros(NWNO), ctx)
    other.zero()
    _lib.check(_lib.load().picaso_memcpy_d2d(ctx, other.addr, d["F0PI"].addr, other.nbytes), ctx)
    assert resident.reflected_seal_stat(ctx)[0] == n1


@pytest.mark.parametrize("how", ["free", "unseal", "memset", "d2d", "pool_trim"])
def test_a_seal_dies_with_its_bytes(ctx, how):
    from picaso_amd import _lib, resident
    d = resident.upload_scene(_scene(), _keys(), ctx=ctx)
    n1 = resident.reflected_seal_stat(ctx)[0]
    lib = _lib.load()
    if how == "free":
        d["w0"].free()
    elif how == "unseal":
        resident.unseal_reflected_planes(ctx, d["cosb_og"].addr + 8 * 17)          # any byte of any plane
    elif how == "memset":
        _lib.check(lib.picaso_memset(ctx, d["gcos2"].addr + 8 * NWNO, 0, 8), ctx)
    elif how == "d2d":
        _lib.check(lib.picaso_memcpy_d2d(ctx, d["dtau_og"].addr, d["dtau"].addr, d["dtau"].nbytes), ctx)
    else:
        _lib.check(lib.picaso_pool_trim(ctx), ctx)
    assert resident.reflected_seal_stat(ctx)[0] == (0 if how == "pool_trim" else n1 - 1)


def test_a_batch_with_an_unsealed_member_keeps_its_planes(monkeypatch, ctx):
    from picaso_amd import resident
    sets = [resident.upload_scene(_scene(21), _keys(), ctx=ctx),
            resident.upload_scene(_scene(22), _keys(), ctx=ctx, seal=False)]
    hits, out, ref = _ab(monkeypatch, ctx, FUSED, lambda: _solve_batch(ctx, sets))
    assert hits == 0
    assert _same(out, ref)


# ------------------------------------------------------------------------------------------------------------------------
# 4. shapes that must not substitute
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [COOP, FUSED], ids=["coop", "fused"])
@pytest.mark.parametrize("kw", [dict(ng=3), dict(single_phase=1), dict(lvl=True)], ids=["three_angles", "single_phase_1",
                                                                                        "get_lvl_flux"])
def test_shapes_without_a_compile_time_variant_keep_their_planes(monkeypatch, ctx, kw, env):
    from picaso_amd import resident
    n0 = resident.reflected_seal_stat(ctx)[0]
    d = resident.upload_scene(_scene(), _keys(), ctx=ctx)
    assert resident.reflected_seal_stat(ctx)[0] == n0 + 1
    hits, out, ref = _ab(monkeypatch, ctx, env, lambda: _solve(ctx, d, **kw))
    assert hits == 0
    assert _same(out, ref)
    assert all(np.isfinite(a).all() for a in out)


@pytest.mark.parametrize("fused_shape", [False, True], ids=["coop", "angle_spread"])
def test_the_small_fused_shapes_keep_their_planes(monkeypatch, ctx, fused_shape):
    """Without the pins of ``FUSED`` a 200-column launch outside the cooperative kernel runs one angle per wave: the
    run-time derived form, which is slower than the eleven-plane kernel."""
    from picaso_amd import resident
    d = resident.upload_scene(_scene(), _keys(), ctx=ctx)
    env = {"PICASO_AMD_REFL_COOP_COLS": "0"} if fused_shape else {}
    hits, out, ref = _ab(monkeypatch, ctx, env, lambda: _solve(ctx, d))
    assert hits == (0 if fused_shape else 1)
    assert _same(out, ref)


def test_a_sharded_upload_seals_at_its_own_pitch(monkeypatch, ctx):
    """Columns [3, 190) of the scene: 187 columns at a pitch of 187 doubles, no multiple of 16 (rows start unaligned)."""
    from picaso_amd import resident
    sc = _scene()
    n0 = resident.reflected_seal_stat(ctx)[0]
    d = resident.upload_scene(sc, _keys(), 3, 190, ctx=ctx)
    assert d["tau"].shape == (NLAYER + 1, 187) and resident.reflected_seal_stat(ctx)[0] == n0 + 1
    hits, out, ref = _ab(monkeypatch, ctx, COOP, lambda: _solve(ctx, d))
    assert hits == 1
    assert _same(out, ref)
    whole = resident.upload_scene(sc, _keys(), ctx=ctx)
    assert np.array_equal(out[1], _solve(ctx, whole)[1][3:190])
