"""Small exponent arguments in the zero-phase reflected sweep (csrc/toon_reflected.hip ``BODY_CLEAR_TOP_SMALL``,
``fexp2_small`` in csrc/device_math.hpp).

A cloud-free layer of the top run whose ``|dtau| <= dt_small = 0.34 min(u)`` in every lane of its wave forms its five
``exp(-dtau/u)`` without range reduction.  That may not move a bit.  Every case compares ``xint_at_top`` and ``albedo`` of a
launch with the same launch under ``PICASO_AMD_REFL_NO_SMALL_EXP=1`` (the switch is read per launch and makes the bound
negative) and with the eleven-plane launch (``PICASO_AMD_REFL_ALL_PLANES=1``), which has no such loop, bit for bit
(compared as 64-bit patterns, so a NaN could not hide either).

The per-lane ``dtau`` values are placed on purpose (``_values``): zeros of both signs, tiny ones, the bound and its
neighbours, the depth at which ``dtau * nl1`` of the smallest angle is exactly -1/2 and its neighbours, and depths far beyond.
A layer is one of three kinds: ``S`` every lane within the bound; ``L`` the lanes cycle through all values; ``M`` wave 0 within
the bound, wave 1 within it but for lane 5 (one ulp above: the vote fails for 63 lanes that would have qualified), the other
waves like ``L``.  ``_kinds(n, p)`` makes layers 0..p small, layer p + 1 ``M`` and lets small layers reappear below large ones,
so the first layer beyond the bound comes after 0, 1, 2, 3 and 4 small layers of the loop (which starts at layer 1 and works
in trips of two: a trip's vote fails on its first or on its second layer), in different waves at different places."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)
FUSED = {"PICASO_AMD_REFL_NO_COOP": "1", "PICASO_AMD_REFL_NO_BIG": "1", "PICASO_AMD_ANGLE_GROUP": "0"}
KNOBS = ("PICASO_AMD_REFL_ALL_PLANES", "PICASO_AMD_REFL_GENERIC", "PICASO_AMD_REFL_COOP_COLS", "PICASO_AMD_MAX_ANGLES",
         "PICASO_AMD_REFL_NO_LAYER_MASK", "PICASO_AMD_REFL_NO_SMALL_EXP") + tuple(FUSED)
NL2E = -1.4426950408889634074
NCOLS = (64, 128, 200, 320)          # one, two, four (ragged) and five waves


def _geometry():
    from picaso_amd import disco
    g, gw, t, tw = disco.get_angles_1d(5)
    u0, u1, _, _, _ = disco.compute_disco(5, 1, g, t, 0.0)
    return u0, u1, gw, tw


def _values():
    """(small, large): the depths within the bound and those beyond it."""
    u = np.asarray(_geometry()[1], dtype=np.float64).ravel()
    umin = float(u.min())
    bound = 0.34 * umin                                   # the launcher's dt_small
    nl1 = NL2E / umin                                     # the kernel's per-angle constant of the smallest angle
    half = 0.5 / -nl1
    for _ in range(8):                                    # the depth whose ROUNDED product is exactly -1/2
        if half * nl1 == -0.5:
            break
        half = np.nextafter(half, np.inf if half * nl1 > -0.5 else 0.0)
    assert half * nl1 == -0.5 and bound * nl1 > -0.4906 and bound < half
    small = [0.0, -0.0, 1e-300, 1e-6, bound, np.nextafter(bound, 0.0), 0.01, 0.09]
    large = [np.nextafter(bound, np.inf), half, np.nextafter(half, 0.0), np.nextafter(half, np.inf), 0.2, 1.0, 40.0]
    return np.array(small), np.array(large)


def _kinds(n, p):
    tail = itertools.cycle("SSLM")
    return (["S"] * (p + 1) + ["M"] + [next(tail) for _ in range(n)])[:n]


def _dtau_row(kind, ncol, shift):
    small, large = _values()
    every = np.concatenate([small, large])
    lane = np.arange(ncol)
    row_s = small[(lane + shift) % len(small)]
    row_l = every[(lane + shift) % len(every)]
    if kind == "S":
        return row_s
    if kind == "L":
        return row_l
    row = np.where(lane < 128, row_s, row_l)
    if ncol > 64:
        row[64 + 5] = large[0]
    else:
        row[5] = large[0]                                 # a single wave: the one lane above the bound sits in it
    return row


def _scene(nlayer, ncol, p, cloudy=(), seed=7):
    """Planes with the layer kinds ``_kinds(nlayer, p)`` in the cloud-free layers and a delta-scaled cloud in ``cloudy``."""
    from picaso_amd import synthetic as syn
    comps = [c.copy() for c in syn.tau_components(nlayer, ncol, syn.BASE_SEED + seed, cloud=False)]
    rng = np.random.default_rng(300 + seed)
    for i in cloudy:
        comps[2][i] = 0.3 * rng.uniform(0.5, 1.5) * (1.0 + 0.3 * np.sin(np.linspace(0.0, 9.0, ncol)))
        comps[3][i] = rng.uniform(0.5, 0.999) * (1.0 - 0.05 * rng.random(ncol))
        comps[4][i] = rng.uniform(0.2, 0.9) * (1.0 - 0.05 * rng.random(ncol))
    sc = syn.mix_planes(*comps)
    kinds = _kinds(nlayer, p)
    for i in range(nlayer):
        if i in cloudy:
            continue
        assert (sc["ftau_cld"][i] == 0).all() and (sc["ftau_ray"][i] == 1).all() and np.array_equal(sc["w0"][i], sc["w0_og"][i])
        sc["dtau"][i] = sc["dtau_og"][i] = _dtau_row(kinds[i], ncol, 3 * i)
    for lv, d in (("tau", "dtau"), ("tau_og", "dtau_og")):         # the level planes stay the running sums
        sc[lv][0] = 0.0
        for i in range(nlayer):
            sc[lv][i + 1] = sc[lv][i] + sc[d][i]
    sc["F0PI"] = np.linspace(0.9, 1.1, ncol)
    sc["surf_reflect"] = np.full(ncol, 0.15)
    return sc


def _keys():
    from picaso_amd import resident
    return resident.REFLECTED_PLANES + ("F0PI", "surf_reflect")


def _solve(ctx, d, planes=None):
    from picaso_amd import device, resident
    nlevel, nwno = d["tau"].shape
    u0, u1, gw, tw = _geometry()
    x, alb = device.DeviceArray((5, 1, nwno), ctx), device.DeviceArray((nwno,), ctx)
    resident.reflected_1d(ctx, nlevel, nwno, 5, 1, d if planes is None else planes, d["surf_reflect"], u0, u1, 1.0,
                          d["F0PI"], 3, 0, *TTHG, x, gweight=gw, tweight=tw, albedo=alb)
    return [x.to_host(), alb.to_host()]


def _solve_batch(ctx, sets, planes):
    from picaso_amd import device, resident
    nlevel, nwno = sets[0]["tau"].shape
    u0, u1, gw, tw = _geometry()
    xs = [device.DeviceArray((5, 1, nwno), ctx) for _ in sets]
    albs = [device.DeviceArray((nwno,), ctx) for _ in sets]
    resident.reflected_1d_batch(ctx, nlevel, nwno, 5, 1, planes, [s["surf_reflect"] for s in sets], u0, u1, 1.0,
                                [s["F0PI"] for s in sets], 3, 0, *TTHG, xs, gweight=gw, tweight=tw, albedo=albs)
    return [a.to_host() for a in xs + albs]


def _same(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and np.array_equal(p, q) and
                                    np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(a, b))


def _pin(monkeypatch, **extra):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(FUSED, **extra).items():
        monkeypatch.setenv(k, v)


def _ab(monkeypatch, run, run_all=None):
    """``run()`` in the fused shape: as it is, with the small-argument loop switched off, and (``run_all``, default ``run``)
    as the eleven-plane launch.  Bit for bit the same; returns the first."""
    _pin(monkeypatch)
    out = run()
    assert all(np.isfinite(a).all() for a in out)
    _pin(monkeypatch, PICASO_AMD_REFL_NO_SMALL_EXP="1")
    off = run()
    _pin(monkeypatch, PICASO_AMD_REFL_ALL_PLANES="1")
    full = (run_all or run)()
    _pin(monkeypatch)
    assert _same(out, off), "differs from the launch with PICASO_AMD_REFL_NO_SMALL_EXP=1"
    assert _same(out, full), "differs from the eleven-plane launch"
    return out


@pytest.fixture
def ctx():
    from picaso_amd import _lib
    return _lib.context()


def _cases():
    out = []
    for j, n in enumerate((1, 2, 3, 4, 5, 8, 12)):
        for p in ((0, 1, 2, 3, 4) if n >= 8 else (0, 1)):
            out.append((n, p, NCOLS[(j + p) % 4]))
    return out


CASES = _cases()
IDS = ["%d_layers_small_to_%d_%d_cols" % c for c in CASES]


def test_the_placed_values():
    small, large = _values()
    u = np.asarray(_geometry()[1], dtype=np.float64).ravel()
    for nl1 in NL2E / u:                                  # within the bound: every angle's rounded product is within 1/2
        assert (np.abs(small * nl1) <= 0.4906).all()
    assert (small <= 0.34 * u.min()).all() and (large > 0.34 * u.min()).all() and large[1] * (NL2E / u.min()) == -0.5
    assert [k for k in "".join(_kinds(12, 2))] == list("SSSMSSLMSSLM")


@pytest.mark.parametrize("nlayer,p,ncol", CASES, ids=IDS)
def test_cloud_free_two_planes(monkeypatch, ctx, nlayer, p, ncol):
    """dtau and w0 alone: the kernel whose whole column is the run."""
    from picaso_amd import resident
    d = resident.upload_scene(_scene(nlayer, ncol, p), _keys(), ctx=ctx, seal=False)
    two = {"dtau": d["dtau"], "w0": d["w0"]}
    _ab(monkeypatch, lambda: _solve(ctx, d, two), lambda: _solve(ctx, d))


@pytest.mark.parametrize("nlayer,p,ncol", CASES, ids=IDS)
def test_eleven_planes_unsealed(monkeypatch, ctx, nlayer, p, ncol):
    from picaso_amd import resident
    d = resident.upload_scene(_scene(nlayer, ncol, p), _keys(), ctx=ctx, seal=False)
    h0 = resident.reflected_seal_stat(ctx)[1]
    _ab(monkeypatch, lambda: _solve(ctx, d))
    assert resident.reflected_seal_stat(ctx)[1] == h0


# (layers, cloudy layers, p): decks of one to three layers at the top, in the middle and at the bottom; the runs under the
# deck have 0, 1, 2, 3 and 5 layers (and 11); the last layer is clear or is not
DECKS = [(12, (0,), 1), (8, (0, 1, 2), 0), (8, (3, 4), 1), (8, (4, 5), 2), (8, (5, 6), 3), (8, (5, 6, 7), 4), (12, (6,), 4),
         (12, (6,), 3), (12, (9, 10, 11), 2), (5, (2,), 0), (5, (4,), 1), (4, (1,), 0), (3, (1,), 0), (3, (2,), 0), (2, (0,), 0),
         (2, (1,), 0), (1, (0,), 0)]


@pytest.mark.parametrize("nlayer,cloudy,p", DECKS, ids=["%d_layers_cloud_%s_small_to_%d" % (n, "_".join(map(str, c)), p)
                                                        for n, c, p in DECKS])
def test_sealed_with_a_cloud_deck(monkeypatch, ctx, nlayer, cloudy, p):
    from picaso_amd import resident
    ncol = NCOLS[(nlayer + p) % 4]
    sc = _scene(nlayer, ncol, p, cloudy)
    assert [int(i) for i in np.flatnonzero((sc["ftau_cld"] != 0).any(axis=1))] == list(cloudy)
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    want = np.array([i not in cloudy for i in range(nlayer)])
    assert np.array_equal(resident.reflected_seal_layers(ctx, d["w0"]), want)
    _pin(monkeypatch)
    m0 = resident.reflected_seal_layers_stat(ctx)
    _ab(monkeypatch, lambda: _solve(ctx, d))
    assert resident.reflected_seal_layers_stat(ctx) - m0 == (2 if want.any() else 0), "on and off take the layers kernel"


def test_batch_small_large_cloud_free(monkeypatch, ctx):
    """Three members: every layer small, every layer large, a cloud-free one handed over whole; each equals its own launch."""
    from picaso_amd import resident
    nlayer, ncol = 8, 200
    scs = [_scene(nlayer, ncol, 7, (5,)), _scene(nlayer, ncol, 0, (5,), seed=8), _scene(nlayer, ncol, 2, seed=9)]
    _, large = _values()
    for i in range(nlayer):
        if i != 5:
            scs[1]["dtau"][i] = scs[1]["dtau_og"][i] = large[(np.arange(ncol) + i) % len(large)]
    for lv, dn in (("tau", "dtau"), ("tau_og", "dtau_og")):
        for i in range(nlayer):
            scs[1][lv][i + 1] = scs[1][lv][i] + scs[1][dn][i]
    assert _kinds(nlayer, 7) == ["S"] * nlayer
    sets = [resident.upload_scene(sc, _keys(), ctx=ctx) for sc in scs]
    out = _ab(monkeypatch, lambda: _solve_batch(ctx, sets, sets))
    for s, d in enumerate(sets):
        own = _ab(monkeypatch, lambda: _solve(ctx, d))
        assert _same([out[s], out[3 + s]], own)
    # ... and three cloud-free members as dtau and w0 alone
    frees = [resident.upload_scene(_scene(nlayer, ncol, p, seed=10 + p), _keys(), ctx=ctx, seal=False) for p in (7, 0, 3)]
    two = [{"dtau": d["dtau"], "w0": d["w0"]} for d in frees]
    out = _ab(monkeypatch, lambda: _solve_batch(ctx, frees, two), lambda: _solve_batch(ctx, frees, frees))
    for s, d in enumerate(frees):
        assert _same([out[s], out[3 + s]], _solve(ctx, d, two[s]))


@pytest.mark.parametrize("shape", [{"PICASO_AMD_REFL_NO_COOP": "0", "PICASO_AMD_REFL_COOP_COLS": "100000"},
                                   {"PICASO_AMD_ANGLE_GROUP": "1"}], ids=["cooperative", "one_angle_per_wave"])
def test_other_launch_shapes_agree(monkeypatch, ctx, shape):
    """The cooperative kernel and the one-angle launch have no small-argument form: a column's result does not depend on
    the launch shape, so they must still give the fused launch's bits."""
    from picaso_amd import resident
    sc = _scene(12, 200, 3, (6,))
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    fused = _ab(monkeypatch, lambda: _solve(ctx, d))
    _pin(monkeypatch)
    for k, v in shape.items():
        if k == "PICASO_AMD_REFL_NO_COOP":
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    other = _solve(ctx, d)
    _pin(monkeypatch)
    assert _same(fused, other)
