"""Runs of cloud-free layers in the zero-phase reflected sweep (csrc/toon_reflected.hip: ``reflected_layer``'s ``XT``,
the top-run loop with ``BODY_CLEAR_TOP``, ``CLEAR_FIRST`` / ``CLEAR_LAST``).

The kernels that form the level sums themselves (``k_reflected_toa<5, false, true, true, false, 2 | 3 | 4>`` and their
batched forms) carry one beam product instead of three while nothing above was delta-scaled, sweep the run of sealed
cloud-free layers from the top in a loop of its own, and give cloud-free first / last layers straight-line copies of the
body.  None of it may change a bit: every case compares ``xint_at_top`` and ``albedo`` of the sealed launch with the same
call under ``PICASO_AMD_REFL_NO_LAYER_MASK=1`` (no run loop, no mask) and under ``PICASO_AMD_REFL_ALL_PLANES=1`` (the
eleven-plane kernel, which has none of the above), asserts through the seal's counters which variant the first launch
took, and asserts from the rows of ``ftau_cld`` that the scene has the layer pattern the case is named after.

200 columns: four waves, the last one partial.  ``FUSED`` pins the shape of the 1e5-column launch.  Scenes are
``synthetic.tau_components`` without cloud, mixed by ``mix_planes``; a cloud slab is put into the first rows and moved to
its layers with ``np.roll``."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)
NWNO = 200
FUSED = {"PICASO_AMD_REFL_COOP_COLS": "0", "PICASO_AMD_ANGLE_GROUP": "0", "PICASO_AMD_REFL_NO_BIG": "1"}
KNOBS = ("PICASO_AMD_REFL_ALL_PLANES", "PICASO_AMD_REFL_GENERIC", "PICASO_AMD_REFL_NO_COOP", "PICASO_AMD_MAX_ANGLES",
         "PICASO_AMD_REFL_NO_LAYER_MASK") + tuple(FUSED)


def _slab(comps, rows, cols, rng):
    """A cloud in the layers ``rows`` (columns ``cols``) of cloud-free components."""
    _, _, taucld, w0c, g0c = comps
    n = taucld[0, cols].shape[0]
    for i in rows:
        taucld[i, cols] = 0.3 * rng.uniform(0.5, 1.5) * (1.0 + 0.3 * np.sin(np.linspace(0.0, 9.0, n)))
        w0c[i, cols] = rng.uniform(0.5, 0.999) * (1.0 - 0.05 * rng.random(n))
        g0c[i, cols] = rng.uniform(0.2, 0.9) * (1.0 - 0.05 * rng.random(n))


def _scene(nlayer, cloudy, seed=41, cols=slice(None)):
    """``cloudy``: the layers that carry cloud.  Contiguous layers are one slab put into rows 0.. and rolled down to its
    place (as the benchmark's distinct batch moves its cloud); scattered layers are one slab each."""
    from picaso_amd import synthetic as syn
    cloudy = sorted(cloudy)
    comps = [c.copy() for c in syn.tau_components(nlayer, NWNO, syn.BASE_SEED + seed, cloud=False)]
    rng = np.random.default_rng(2000 + seed)
    slabs, run = [], []
    for i in cloudy:
        if run and i != run[-1] + 1:
            slabs.append(run)
            run = []
        run.append(i)
    if run:
        slabs.append(run)
    cloud = [np.zeros_like(c) for c in comps[2:]]
    for sl in slabs:
        part = [None, None] + [np.zeros_like(c) for c in comps[2:]]
        _slab(part, range(len(sl)), cols, rng)
        for acc, p in zip(cloud, part[2:]):
            acc += np.roll(p, sl[0], axis=0)
    comps[2:] = cloud
    sc = syn.mix_planes(*comps)
    sc["F0PI"] = np.linspace(0.9, 1.1, NWNO)
    sc["surf_reflect"] = np.full(NWNO, 0.15)
    return sc


def _cloud_rows(sc):
    """The layers with cloud in any column, from the rows of ``ftau_cld``."""
    return [int(i) for i in np.flatnonzero((sc["ftau_cld"] != 0.0).any(axis=1))]


def _keys():
    from picaso_amd import resident
    return resident.REFLECTED_PLANES + ("F0PI", "surf_reflect")


def _geometry():
    from picaso_amd import disco
    g, gw, t, tw = disco.get_angles_1d(5)
    u0, u1, _, _, _ = disco.compute_disco(5, 1, g, t, 0.0)
    return u0, u1, gw, tw


def _solve(ctx, d, planes=None):
    """One five-angle ``reflected_1d`` on the resident set ``d`` (``planes``: the ones handed over): [xint, albedo]."""
    from picaso_amd import device, resident
    nlevel, nwno = d["tau"].shape
    u0, u1, gw, tw = _geometry()
    x, alb = device.DeviceArray((5, 1, nwno), ctx), device.DeviceArray((nwno,), ctx)
    resident.reflected_1d(ctx, nlevel, nwno, 5, 1, d if planes is None else planes, d["surf_reflect"], u0, u1, 1.0,
                          d["F0PI"], 3, 0, *TTHG, x, gweight=gw, tweight=tw, albedo=alb)
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
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def _pin(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FUSED.items():
        monkeypatch.setenv(k, v)


def _abc(monkeypatch, ctx, run):
    """``run()`` in the pinned fused shape as it is (a), with ``PICASO_AMD_REFL_NO_LAYER_MASK=1`` (b) and with
    ``PICASO_AMD_REFL_ALL_PLANES=1`` (c); all three bit for bit the same.  Returns (mask launches, seal hits, outputs) of
    (a)."""
    from picaso_amd import resident
    _pin(monkeypatch)
    m0, h0 = resident.reflected_seal_layers_stat(ctx), resident.reflected_seal_stat(ctx)[1]
    out = run()
    masks, hits = resident.reflected_seal_layers_stat(ctx) - m0, resident.reflected_seal_stat(ctx)[1] - h0
    assert all(np.isfinite(a).all() for a in out) and all(a.max() > 0 for a in out)
    monkeypatch.setenv("PICASO_AMD_REFL_NO_LAYER_MASK", "1")
    ref_levels = run()
    monkeypatch.delenv("PICASO_AMD_REFL_NO_LAYER_MASK")
    assert resident.reflected_seal_stat(ctx)[1] == h0 + 2 * hits, "the switch turns the mask off, not the seal"
    monkeypatch.setenv("PICASO_AMD_REFL_ALL_PLANES", "1")
    ref_all = run()
    monkeypatch.delenv("PICASO_AMD_REFL_ALL_PLANES")
    assert resident.reflected_seal_layers_stat(ctx) == m0 + masks, "the reference runs must not use a mask"
    assert _same(out, ref_levels), "differs from the sealed launch without the mask"
    assert _same(out, ref_all), "differs from the all-planes launch"
    return masks, hits, out


def _check(monkeypatch, ctx, nlayer, cloudy, **kw):
    """The scene with cloud in ``cloudy``: it has that pattern, the seal's mask is its complement, the launch takes the
    layers variant exactly when a clear layer exists and the three launches agree."""
    from picaso_amd import resident
    sc = _scene(nlayer, cloudy, **kw)
    cloudy = sorted(cloudy)
    assert sc["dtau"].shape == (nlayer, NWNO) and _cloud_rows(sc) == cloudy, "the scene does not exercise its case"
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    want = np.array([i not in cloudy for i in range(nlayer)])
    got = resident.reflected_seal_layers(ctx, d["w0"])
    if nlayer <= 128:
        assert got is not None and np.array_equal(got, want)
    else:
        assert got is None
    masks, hits, out = _abc(monkeypatch, ctx, lambda: _solve(ctx, d))
    assert hits == 1
    assert masks == (1 if (nlayer <= 128 and want.any()) else 0)
    return sc, d, out


@pytest.fixture
def ctx():
    from picaso_amd import _lib
    return _lib.context()


# ------------------------------------------------------------------------------------------------------------------------
# 1. layer counts: the one-layer path, both parities of the loop over two register sets, its tail
# ------------------------------------------------------------------------------------------------------------------------
COUNTS = [(n, kind) for n in (1, 2, 3, 4, 7) for kind in ("no_clear_layer", "all_clear", "one_cloudy_layer")]


@pytest.mark.parametrize("nlayer,kind", COUNTS, ids=["%d_%s" % c for c in COUNTS])
def test_layer_counts(monkeypatch, ctx, nlayer, kind):
    cloudy = {"no_clear_layer": list(range(nlayer)), "all_clear": [], "one_cloudy_layer": [nlayer // 2]}[kind]
    _check(monkeypatch, ctx, nlayer, cloudy)


# ------------------------------------------------------------------------------------------------------------------------
# 2. where the cloud sits: empty top run, general last layer, a deck with clear layers below it (S_EO != S_XU there)
# ------------------------------------------------------------------------------------------------------------------------
def _positions(n):
    return {"layer_0_only": [0], "last_layer_only": [n - 1], "layers_3_4": [3, 4], "layer_0_and_last": [0, n - 1],
            "alternating_odd_cloudy": list(range(1, n, 2)), "alternating_even_cloudy": list(range(0, n, 2))}


@pytest.mark.parametrize("name", list(_positions(7)))
@pytest.mark.parametrize("nlayer", [7, 8])
def test_cloud_positions(monkeypatch, ctx, nlayer, name):
    _check(monkeypatch, ctx, nlayer, _positions(nlayer)[name])


def test_a_layer_cloudy_in_one_wave_only(monkeypatch, ctx):
    """Layer 2 carries cloud in columns [0, 64) only: not in the mask, so it ends the top run, yet three of the four waves
    pass the vote there and take the cloud-free copy of the masked loop."""
    sc, _, _ = _check(monkeypatch, ctx, 7, [2], cols=slice(0, 64))
    assert (sc["ftau_cld"][2, :64] > 0).all() and (sc["ftau_cld"][2, 64:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------
# 3. the second mask word; more layers than a mask holds
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlayer,cloudy", [(66, [64, 65]), (70, [10])], ids=["66_cloud_64_65", "70_cloud_10"])
def test_second_mask_word(monkeypatch, ctx, nlayer, cloudy):
    _check(monkeypatch, ctx, nlayer, cloudy)


def test_129_layers_run_without_mask(monkeypatch, ctx):
    _check(monkeypatch, ctx, 129, [64])


# ------------------------------------------------------------------------------------------------------------------------
# 4. DRV = 2: a cloud-free atmosphere handed over as dtau and w0 alone
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlayer", [1, 2, 3, 4, 7, 8])
def test_only_dtau_and_w0(monkeypatch, ctx, nlayer):
    from picaso_amd import resident
    sc = _scene(nlayer, [])
    assert _cloud_rows(sc) == [] and np.array_equal(sc["dtau_og"], sc["dtau"]) and np.array_equal(sc["w0_og"], sc["w0"])
    d = resident.upload_scene(sc, _keys(), ctx=ctx, seal=False)
    _pin(monkeypatch)
    h0 = resident.reflected_seal_stat(ctx)[1]
    two = _solve(ctx, d, planes={"dtau": d["dtau"], "w0": d["w0"]})
    monkeypatch.setenv("PICASO_AMD_REFL_ALL_PLANES", "1")
    ref = _solve(ctx, d)
    monkeypatch.delenv("PICASO_AMD_REFL_ALL_PLANES")
    assert resident.reflected_seal_stat(ctx)[1] == h0          # no seal involved on either side
    assert np.isfinite(two[1]).all() and (two[1] > 0).all()
    assert _same(two, ref)


# ------------------------------------------------------------------------------------------------------------------------
# 5. batched: every member with its own mask and run length
# ------------------------------------------------------------------------------------------------------------------------
def test_batch_of_four_run_lengths(monkeypatch, ctx):
    from picaso_amd import resident
    members = {"top_run_only": [5, 6], "deck_in_the_middle": [3], "cloud_in_layer_0": [0], "no_cloud": []}
    sets = []
    for m, cloudy in enumerate(members.values()):
        sc = _scene(7, cloudy, seed=41 + m)
        assert _cloud_rows(sc) == cloudy
        sets.append(resident.upload_scene(sc, _keys(), ctx=ctx))
    masks, hits, out = _abc(monkeypatch, ctx, lambda: _solve_batch(ctx, sets))
    assert (masks, hits) == (1, 1)
    for s, d in enumerate(sets):
        m, _, own = _abc(monkeypatch, ctx, lambda: _solve(ctx, d))
        assert m == 1
        assert _same([out[s], out[4 + s]], own)
