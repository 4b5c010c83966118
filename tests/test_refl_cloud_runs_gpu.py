"""Run loops for sealed cloud decks and the small-argument ``EP`` of the zero-phase reflected sweep
(csrc/toon_reflected.hip: the cloud-run loop of the ``DRV = 4`` kernels, ``BODY_CLEAR_TOP_SMALL_EP``).

A seal records, beside its clear-layer mask, which layers are cloudy and delta-scaled in EVERY column (``!(ftau_cld == 0)``
and ``!(dtau_og == dtau)``, the solver's own two comparisons negated) and whether every ``w0`` lies in [0, 1].  The fused
five-angle launch sweeps a run of such deck layers two per trip by ``BODY_CLOUD`` without votes, mask tests or dispatch, and
forms ``EP = 2^(lam dtau log2 e)`` of a small top-run layer without range reduction when the ``w0`` fact holds and the angle
table is small enough (``0.34 min(u) sqrt(3) log2(e) <= 1/2``).  None of that may move a bit.  Every case compares
``xint_at_top`` and ``albedo``, as 64-bit patterns, between the launch itself, the same launch under
``PICASO_AMD_REFL_NO_CLOUD_RUNS=1`` (both off, read per launch), under ``PICASO_AMD_REFL_NO_LAYER_MASK=1`` (the ``DRV = 3``
kernel: every layer votes) and under ``PICASO_AMD_REFL_ALL_PLANES=1`` (the eleven-plane kernel, which has none of this).

The two facts are private to the seal -- no export hands them out -- so a case cannot read a bit of the deck mask or the flag;
what it can see is that a layer the loop must not take (one column without cloud, one column not delta-scaled) and a set
whose flag must be off (a ``w0`` outside [0, 1], a table of larger angles) give the bits of the launches that have neither.
A NaN in ``ftau_cld`` is cloudy to the solver's votes (``NaN == 0`` fails) and so, by the same comparison, to the seal: the
layer stays in the run and must give the other launches' bits, NaN column included.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)
FUSED = {"PICASO_AMD_REFL_NO_COOP": "1", "PICASO_AMD_REFL_NO_BIG": "1", "PICASO_AMD_ANGLE_GROUP": "0"}
KNOBS = ("PICASO_AMD_REFL_ALL_PLANES", "PICASO_AMD_REFL_GENERIC", "PICASO_AMD_REFL_COOP_COLS", "PICASO_AMD_MAX_ANGLES",
         "PICASO_AMD_REFL_NO_LAYER_MASK", "PICASO_AMD_REFL_NO_SMALL_EXP", "PICASO_AMD_REFL_NO_CLOUD_RUNS") + tuple(FUSED)
NCOLS = (64, 130, 320)               # one wave, two full waves and two lanes of a third, five waves
SQ3, LOG2E = 1.7320508075688772935, 1.4426950408889634074
ODD = 64 + 5                         # wave 1, lane 5 (a single wave: lane 5)


def _geometry(u=None):
    from picaso_amd import disco
    g, gw, t, tw = disco.get_angles_1d(5)
    u0, u1, _, _, _ = disco.compute_disco(5, 1, g, t, 0.0)
    if u is not None:                                     # a symmetric table with one angle five times
        u0 = np.full_like(np.asarray(u0, dtype=np.float64), u)
        u1 = u0.copy()
    return u0, u1, gw, tw


def _resum(sc):
    """The level planes stay the running sums (what a seal verifies)."""
    for lv, d in (("tau", "dtau"), ("tau_og", "dtau_og")):
        sc[lv][0] = 0.0
        for i in range(sc[d].shape[0]):
            sc[lv][i + 1] = sc[lv][i] + sc[d][i]


def _scene(nlayer, ncol, cloudy, seed=11, dt_clear=None, w0_clear=None):
    """A delta-scaled cloud in the layers ``cloudy`` (every column), no cloud elsewhere.  ``dt_clear`` / ``w0_clear``: per-lane
    values for the cloud-free layers (``dt_clear`` shifted from layer to layer, ``w0_clear`` the same in every layer)."""
    from picaso_amd import synthetic as syn
    comps = [c.copy() for c in syn.tau_components(nlayer, ncol, syn.BASE_SEED + seed, cloud=False)]
    rng = np.random.default_rng(500 + seed)
    for i in cloudy:
        comps[2][i] = 0.3 * rng.uniform(0.5, 1.5) * (1.0 + 0.3 * np.sin(np.linspace(0.0, 9.0, ncol)))
        comps[3][i] = rng.uniform(0.5, 0.999) * (1.0 - 0.05 * rng.random(ncol))
        comps[4][i] = rng.uniform(0.2, 0.9) * (1.0 - 0.05 * rng.random(ncol))
    sc = syn.mix_planes(*comps)
    lane = np.arange(ncol)
    for i in range(nlayer):
        if i in cloudy:
            assert (sc["ftau_cld"][i] != 0).all() and (sc["dtau_og"][i] != sc["dtau"][i]).all()
            continue
        assert (sc["ftau_cld"][i] == 0).all() and (sc["ftau_ray"][i] == 1).all() and np.array_equal(sc["w0"][i], sc["w0_og"][i])
        if dt_clear is not None:
            sc["dtau"][i] = sc["dtau_og"][i] = np.asarray(dt_clear)[(lane + 3 * i) % len(dt_clear)]
        if w0_clear is not None:
            sc["w0"][i] = sc["w0_og"][i] = np.asarray(w0_clear)[lane % len(w0_clear)]      # a column keeps its value
    _resum(sc)
    sc["F0PI"] = np.linspace(0.9, 1.1, ncol)
    sc["surf_reflect"] = np.full(ncol, 0.15)
    return sc


def _keys():
    from picaso_amd import resident
    return resident.REFLECTED_PLANES + ("F0PI", "surf_reflect")


def _solve(ctx, d, u=None):
    from picaso_amd import device, resident
    nlevel, nwno = d["tau"].shape
    u0, u1, gw, tw = _geometry(u)
    x, alb = device.DeviceArray((5, 1, nwno), ctx), device.DeviceArray((nwno,), ctx)
    resident.reflected_1d(ctx, nlevel, nwno, 5, 1, d, d["surf_reflect"], u0, u1, 1.0, d["F0PI"], 3, 0, *TTHG, x,
                          gweight=gw, tweight=tw, albedo=alb)
    return [x.to_host(), alb.to_host()]


def _solve_batch(ctx, sets):
    from picaso_amd import device, resident
    nlevel, nwno = sets[0]["tau"].shape
    u0, u1, gw, tw = _geometry()
    xs = [device.DeviceArray((5, 1, nwno), ctx) for _ in sets]
    albs = [device.DeviceArray((nwno,), ctx) for _ in sets]
    resident.reflected_1d_batch(ctx, nlevel, nwno, 5, 1, sets, [s["surf_reflect"] for s in sets], u0, u1, 1.0,
                                [s["F0PI"] for s in sets], 3, 0, *TTHG, xs, gweight=gw, tweight=tw, albedo=albs)
    return [a.to_host() for a in xs + albs]


def _same(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and np.array_equal(p.view(np.uint64), q.view(np.uint64))
                                    for p, q in zip(a, b))


def _pin(monkeypatch, **extra):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(FUSED, **extra).items():
        monkeypatch.setenv(k, v)


def _ab(monkeypatch, ctx, run, finite=True):
    """``run()`` in the fused shape: as it is, without cloud runs and small EP, without the layer masks, and as the eleven-
    plane launch.  Bit for bit the same; the first two take the layers kernel.  Returns the first."""
    from picaso_amd import resident
    _pin(monkeypatch)
    m0 = resident.reflected_seal_layers_stat(ctx)
    out = run()
    took = resident.reflected_seal_layers_stat(ctx) - m0
    if finite:
        assert all(np.isfinite(a).all() for a in out)
    others = {}
    for knob in ("PICASO_AMD_REFL_NO_CLOUD_RUNS", "PICASO_AMD_REFL_NO_LAYER_MASK", "PICASO_AMD_REFL_ALL_PLANES"):
        _pin(monkeypatch, **{knob: "1"})
        m0 = resident.reflected_seal_layers_stat(ctx)
        others[knob] = run()
        if knob == "PICASO_AMD_REFL_NO_CLOUD_RUNS":
            assert resident.reflected_seal_layers_stat(ctx) - m0 == took, "the switch keeps the kernel"
    _pin(monkeypatch)
    for knob, res in others.items():
        assert _same(out, res), "differs from the launch with %s=1" % knob
    return out, took


@pytest.fixture
def ctx():
    from picaso_amd import _lib
    return _lib.context()


# (layers, deck layers): a deck at layer 0 and one ending at n - 1; decks of 1, 2, 3 and 4 layers starting at even and at
# odd layers; a deck directly below a top run of 0, 1, 2 and 3 layers; two decks 0, 1, 2 and 3 clear layers apart; every
# layer cloudy.  Layers run from 3 to 14.
DECKS = [
    (8, (0,)), (9, (0, 1)), (10, (0, 1, 2)), (11, (0, 1, 2, 3)),                   # top run of 0 layers, lengths 1..4
    (12, (1,)), (12, (1, 2)), (13, (1, 2, 3)), (14, (1, 2, 3, 4)),                 # top run of 1: odd start
    (12, (2,)), (12, (2, 3)), (13, (2, 3, 4)), (14, (2, 3, 4, 5)),                 # top run of 2: even start
    (12, (3,)), (12, (3, 4)), (13, (3, 4, 5)), (14, (3, 4, 5, 6)),                 # top run of 3
    (12, (6, 7, 8, 9)), (12, (5, 6, 7, 8)),                                       # deep decks, even and odd start
    (8, (7,)), (9, (7, 8)), (10, (7, 8, 9)), (12, (8, 9, 10, 11)), (11, (7, 8, 9, 10)),   # ending at n - 1
    (14, (2, 3, 4, 5, 6, 7)),                                                     # two decks 0 apart are one
    (14, (2, 3, 4, 6, 7, 8)), (14, (3, 4, 5, 6, 8, 9)),                           # 1 apart
    (14, (2, 3, 4, 7, 8, 9)), (14, (1, 2, 5, 6, 7, 8)),                           # 2 apart
    (14, (2, 3, 4, 8, 9, 10)), (14, (1, 2, 3, 4, 8, 9, 10, 11)),                  # 3 apart
    (3, (0, 1, 2)), (4, (0, 1, 2, 3)), (7, tuple(range(7))), (14, tuple(range(14))),      # every layer cloudy
    (3, (1,)), (4, (1, 2)), (5, (1, 2, 3)), (6, (1, 2, 3, 4)), (5, (0, 1, 2, 3)),   # short columns
]


@pytest.mark.parametrize("nlayer,cloudy", DECKS, ids=["%d_layers_deck_%s" % (n, "_".join(map(str, c))) for n, c in DECKS])
def test_deck_patterns(monkeypatch, ctx, nlayer, cloudy):
    from picaso_amd import resident
    ncol = NCOLS[(nlayer + len(cloudy) + cloudy[0]) % 3]
    sc = _scene(nlayer, ncol, cloudy)
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    want = np.array([i not in cloudy for i in range(nlayer)])
    assert np.array_equal(resident.reflected_seal_layers(ctx, d["w0"]), want)
    _, took = _ab(monkeypatch, ctx, lambda: _solve(ctx, d))
    assert took == (1 if want.any() else 0), "a set with a clear layer takes the layers kernel"


ODDS = ["ftau_cld_zero", "not_delta_scaled", "ftau_cld_nan"]


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("odd", ODDS)
def test_one_odd_column_in_a_deck(monkeypatch, ctx, odd, ncol):
    """Layers 3..8 of 12 carry the deck; in layers 4 (second of a trip) and 7 (first of one) one column differs."""
    from picaso_amd import resident
    sc = _scene(12, ncol, (3, 4, 5, 6, 7, 8), seed=12)
    col = ODD if ncol > 64 else 5
    for i in (4, 7):
        if odd == "ftau_cld_zero":
            sc["ftau_cld"][i, col] = 0.0
        elif odd == "not_delta_scaled":
            sc["dtau_og"][i, col] = sc["dtau"][i, col]
        else:
            sc["ftau_cld"][i, col] = np.nan
    _resum(sc)
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    assert np.array_equal(resident.reflected_seal_layers(ctx, d["w0"]), np.array([i < 3 or i > 8 for i in range(12)]))
    out, took = _ab(monkeypatch, ctx, lambda: _solve(ctx, d), finite=odd != "ftau_cld_nan")
    assert took == 1
    if odd == "ftau_cld_nan":                           # the NaN stays in its column
        bad = ~np.isfinite(out[0]).all(axis=(0, 1))
        assert bad[col] and bad.sum() == 1 and np.array_equal(~np.isfinite(out[1]), bad)


def _ep_depths(u):
    """dt_small of a table with smallest angle ``u``, and the depth whose rounded E log2(e) lies closest below 1/2 for
    w0 = 0 (lam = sqrt(3) as the kernel forms it: fl(sqrt(3)/2) * 2, squared, rooted)."""
    bound = 0.34 * u
    lam = np.sqrt((SQ3 * 0.5 * 2.0) ** 2)
    dt = 0.5 / (lam * LOG2E)
    for _ in range(64):
        if (lam * dt) * LOG2E < 0.5:
            break
        dt = np.nextafter(dt, 0.0)
    while (lam * np.nextafter(dt, np.inf)) * LOG2E < 0.5:
        dt = np.nextafter(dt, np.inf)
    assert (lam * dt) * LOG2E < 0.5 <= (lam * np.nextafter(dt, np.inf)) * LOG2E
    return bound, dt


W0_IN = [0.0, 1e-9, 1.0, 0.3, 0.999]
EP_CASES = [("gauss", None, W0_IN, 64), ("gauss", None, W0_IN, 320), ("u_058", 0.58, W0_IN, 130), ("u_060", 0.60, W0_IN, 130),
            ("u_058", 0.58, W0_IN + [np.nextafter(1.0, 2.0)], 130), ("u_058", 0.58, W0_IN + [-1e-3], 130),
            ("gauss", None, W0_IN + [np.nextafter(1.0, 2.0)], 320), ("gauss", None, W0_IN + [-1e-3], 64)]


@pytest.mark.parametrize("table,u,w0s,ncol", EP_CASES,
                         ids=["%s_%s_%d_cols" % (t, "unit_w0" if len(w) == len(W0_IN) else "w0_%g" % w[-1], c)
                              for t, _, w, c in EP_CASES])
def test_small_ep(monkeypatch, ctx, table, u, w0s, ncol):
    """A top run of nine small layers over a two-layer deck, w0 of 0, 1e-9 and 1 among the lanes; dtau at dt_small, just
    below it and tiny.  A column with w0 = 0 (g2 = 0: Gamma is NaN, as in the reference's (g1 - lamda)/g2), w0 = 1 (lam = 0)
    or a w0 outside [0, 1] need not be finite -- its bit patterns are compared like all others; every other column is.
    Layer 6 holds, in one lane, the depth closest below E log2(e) = 1/2 (beyond dt_small in every table the flag allows:
    its trip leaves the small loop).  u = 0.58: 0.34 u sqrt(3) log2(e) = 0.4928, flag on;
    u = 0.60: 0.5098, flag off; a w0 above 1 or below 0 anywhere in the set: flag off."""
    from picaso_amd import resident
    umin = float(np.asarray(_geometry(u)[1]).min())
    bound, half = _ep_depths(umin)
    assert (0.34 * umin * SQ3 * LOG2E * (1.0 + 2.0 ** -40) <= 0.5) == (table != "u_060")
    assert (half > bound) == (table != "u_060")          # u = 0.60: that depth passes the vote, and EP keeps its general form
    small = [bound, np.nextafter(bound, 0.0), 0.5 * bound, 1e-6, 0.0, 1e-300]
    sc = _scene(14, ncol, (10, 11), seed=13, dt_clear=small, w0_clear=w0s)
    col = ODD if ncol > 64 else 5
    sc["dtau"][6, col] = sc["dtau_og"][6, col] = half
    sc["w0"][6, col] = sc["w0_og"][6, col] = 0.0
    _resum(sc)
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    out, took = _ab(monkeypatch, ctx, lambda: _solve(ctx, d, u), finite=False)
    assert took == 1
    w0col = np.asarray(w0s)[np.arange(ncol) % len(w0s)]
    good = (w0col > 0.0) & (w0col < 1.0)
    good[col] = False
    assert good.sum() >= ncol // 3 and np.isfinite(out[0][..., good]).all() and np.isfinite(out[1][good]).all()


def test_batch_members_with_different_masks(monkeypatch, ctx):
    """Four members: decks in different places, one without cloud, one with a w0 above 1 (the flag is the launch's: off for
    all); each equals its own launch."""
    from picaso_amd import resident
    nlayer, ncol = 12, 130
    small = [0.003, 0.01, 1e-6, 0.0]
    scs = [_scene(nlayer, ncol, (3, 4, 5, 6), seed=20, dt_clear=small), _scene(nlayer, ncol, (0, 1, 7, 8, 9), seed=21),
           _scene(nlayer, ncol, (), seed=22, dt_clear=small), _scene(nlayer, ncol, (4, 5), seed=23, dt_clear=small)]
    sets = [resident.upload_scene(sc, _keys(), ctx=ctx) for sc in scs]
    out, took = _ab(monkeypatch, ctx, lambda: _solve_batch(ctx, sets))
    assert took == 1
    for s, d in enumerate(sets):
        own, _ = _ab(monkeypatch, ctx, lambda: _solve(ctx, d))
        assert _same([out[s], out[len(sets) + s]], own)
    scs[3]["w0"][1, 7] = scs[3]["w0_og"][1, 7] = np.nextafter(1.0, 2.0)
    sets[3] = resident.upload_scene(scs[3], _keys(), ctx=ctx)
    out2, _ = _ab(monkeypatch, ctx, lambda: _solve_batch(ctx, sets), finite=False)
    assert _same(out2[:3], out[:3])
