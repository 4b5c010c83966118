"""Clear-layer masks of sealed reflected plane sets (csrc/planeseal.hip, ``k_reflected_toa<5, false, true, true, false, 4>``
and its batched form in csrc/toon_reflected.hip, the launcher in csrc/api.hip).

The seal records which layers carry no cloud in any column; the fused five-angle launch then reads ``dtau`` and ``w0``
alone in those layers and puts the other values in.  What is checked here: the mask equals the one numpy finds in the
host planes, the variant is taken exactly when a mask with a clear layer exists (``picaso_reflected_seal_layers_stat``),
and every solve returns the bits of the same resident set run with ``PICASO_AMD_REFL_NO_LAYER_MASK=1`` (the sealed launch
without the mask) and with ``PICASO_AMD_REFL_ALL_PLANES=1`` (all eleven planes).

Scenes come from ``synthetic.tau_components`` without cloud; the cloud rows are put in by hand.  600 columns: two full
workgroups and a third of one full wave and a 24-lane wave.  ``FUSED`` pins the shape of the 1e5-column launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)
NWNO = 600
FUSED = {"PICASO_AMD_REFL_COOP_COLS": "0", "PICASO_AMD_ANGLE_GROUP": "0", "PICASO_AMD_REFL_NO_BIG": "1"}
KNOBS = ("PICASO_AMD_REFL_ALL_PLANES", "PICASO_AMD_REFL_GENERIC", "PICASO_AMD_REFL_NO_COOP", "PICASO_AMD_MAX_ANGLES",
         "PICASO_AMD_REFL_NO_LAYER_MASK") + tuple(FUSED)


def _components(nlayer, cloudy, nwno=NWNO, seed=31):
    """Cloud-free tau components with a cloud put into the layers ``cloudy`` (all columns)."""
    from picaso_amd import synthetic as syn
    comps = [c.copy() for c in syn.tau_components(nlayer, nwno, syn.BASE_SEED + seed, cloud=False)]
    rng = np.random.default_rng(1000 + seed)
    for i in cloudy:
        _cloud_row(comps, i, slice(None), rng)
    return comps


def _cloud_row(comps, i, cols, rng):
    _, _, taucld, w0c, g0c = comps
    n = taucld[i, cols].shape[0]
    taucld[i, cols] = 0.3 * rng.uniform(0.5, 1.5) * (1.0 + 0.3 * np.sin(np.linspace(0.0, 9.0, n)))
    w0c[i, cols] = rng.uniform(0.5, 0.999) * (1.0 - 0.05 * rng.random(n))
    g0c[i, cols] = rng.uniform(0.2, 0.9) * (1.0 - 0.05 * rng.random(n))


def _mix(comps):
    from picaso_amd import synthetic as syn
    sc = syn.mix_planes(*comps)
    nwno = sc["dtau"].shape[1]
    sc["F0PI"] = np.linspace(0.9, 1.1, nwno)
    sc["surf_reflect"] = np.full(nwno, 0.15)
    return sc


def _scene(nlayer, cloudy, nwno=NWNO, seed=31):
    return _mix(_components(nlayer, cloudy, nwno, seed))


def _resum(sc):
    """``tau`` / ``tau_og`` as the running sums of the (edited) layer depths and ``gcos2 = 0.5 ftau_ray``: the set seals."""
    for lvl, lay in (("tau", "dtau"), ("tau_og", "dtau_og")):
        sc[lvl][0] = 0.0
        for i in range(sc[lay].shape[0]):
            sc[lvl][i + 1] = sc[lvl][i] + sc[lay][i]
    sc["gcos2"] = 0.5 * sc["ftau_ray"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _np_mask(sc, lo=None, hi=None):
    """The four conditions of a clear layer, over the columns [lo, hi)."""
    c = slice(lo, hi)
    ok = (sc["ftau_cld"][:, c] == 0.0) & (sc["dtau_og"][:, c] == sc["dtau"][:, c]) & \
        (_bits(sc["ftau_ray"][:, c]) == _bits(np.ones(1))[0]) & (_bits(sc["w0_og"][:, c]) == _bits(sc["w0"][:, c]))
    return ok.all(axis=1)


def _keys():
    from picaso_amd import resident
    return resident.REFLECTED_PLANES + ("F0PI", "surf_reflect")


def _geometry():
    from picaso_amd import disco
    g, gw, t, tw = disco.get_angles_1d(5)
    u0, u1, _, _, _ = disco.compute_disco(5, 1, g, t, 0.0)
    return u0, u1, gw, tw


def _solve(ctx, d):
    """One five-angle ``reflected_1d`` on the resident set ``d``: [xint, albedo] as host arrays."""
    from picaso_amd import device, resident
    nlevel, nwno = d["tau"].shape
    u0, u1, gw, tw = _geometry()
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
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def _abc(monkeypatch, ctx, run):
    """``run()`` in the pinned fused shape three times: as it is, with ``PICASO_AMD_REFL_NO_LAYER_MASK=1`` and with
    ``PICASO_AMD_REFL_ALL_PLANES=1``.  Asserts that the three agree bit for bit and that the two references used no
    mask; returns (mask launches, seal hits, outputs) of the first run."""
    from picaso_amd import resident
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FUSED.items():
        monkeypatch.setenv(k, v)
    m0, h0 = resident.reflected_seal_layers_stat(ctx), resident.reflected_seal_stat(ctx)[1]
    out = run()
    masks, hits = resident.reflected_seal_layers_stat(ctx) - m0, resident.reflected_seal_stat(ctx)[1] - h0
    assert all(np.isfinite(a).all() for a in out)
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


def _check(monkeypatch, ctx, sc, want_variant=True, lo=None, hi=None):
    """Upload (sealing), compare the mask with numpy's and the solve with its two references."""
    from picaso_amd import resident
    d = resident.upload_scene(sc, _keys(), lo, hi, ctx=ctx)
    want = _np_mask(sc, lo, hi)
    got = resident.reflected_seal_layers(ctx, d["w0"].addr + 8)
    assert got is not None and np.array_equal(got, want)
    masks, hits, out = _abc(monkeypatch, ctx, lambda: _solve(ctx, d))
    assert hits == 1
    assert masks == (1 if want_variant else 0)
    assert want.any() == want_variant
    return d, out


@pytest.fixture
def ctx():
    from picaso_amd import _lib
    return _lib.context()


# ------------------------------------------------------------------------------------------------------------------------
# 1., 2. the mask, and the layer patterns at six layers
# ------------------------------------------------------------------------------------------------------------------------
PATTERNS = {
    "cloud_in_first_layer": [0],                 # the peeled first layer is the cloudy one
    "cloud_in_last_layer": [5],                  # the peeled last layer
    "alternating_even_cloudy": [0, 2, 4],        # the two register sets: one always loads eight rows, the other two
    "alternating_odd_cloudy": [1, 3, 5],
    "cloud_in_two_interior_layers": [2, 3],
    "all_clear": [],
}


@pytest.mark.parametrize("name", list(PATTERNS))
def test_layer_patterns(monkeypatch, ctx, name):
    sc = _scene(6, PATTERNS[name])
    assert np.array_equal(_np_mask(sc), [i not in PATTERNS[name] for i in range(6)])
    _check(monkeypatch, ctx, sc)


def test_no_clear_layer_runs_the_sealed_launch_without_mask(monkeypatch, ctx):
    sc = _scene(6, range(6))
    assert not _np_mask(sc).any()
    _check(monkeypatch, ctx, sc, want_variant=False)


# ------------------------------------------------------------------------------------------------------------------------
# 3. layer counts: the one-layer path, odd and even tails of the loop unrolled by two, the word boundary of the mask
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlayer,cloudy", [(1, []), (1, [0]), (2, [1]), (3, [1]), (64, [32]), (65, [32, 64]), (65, [63]),
                                           (128, [64]), (128, [127])])
def test_layer_counts(monkeypatch, ctx, nlayer, cloudy):
    _check(monkeypatch, ctx, _scene(nlayer, cloudy), want_variant=len(cloudy) < nlayer)


def test_more_than_128_layers_record_no_mask(monkeypatch, ctx):
    from picaso_amd import resident
    sc = _scene(129, [64])
    d = resident.upload_scene(sc, _keys(), ctx=ctx)
    assert resident.seal_reflected_planes(ctx, 130, NWNO, d) == 7
    assert resident.reflected_seal_layers(ctx, d["dtau"]) is None
    masks, hits, _ = _abc(monkeypatch, ctx, lambda: _solve(ctx, d))
    assert (masks, hits) == (0, 1)


# ------------------------------------------------------------------------------------------------------------------------
# 4., 5. near misses in one column leave the layer unflagged; -0.0 in ftau_cld
# ------------------------------------------------------------------------------------------------------------------------
def _tiny_cloud(sc, i, j):
    sc["ftau_cld"][i, j] = 1e-300


def _ray_below_one(sc, i, j):
    sc["ftau_ray"][i, j] = np.nextafter(1.0, 0.0)


def _w0_og_ulp(sc, i, j):
    sc["w0_og"][i, j] = np.nextafter(sc["w0"][i, j], 0.0)


def _dtau_og_ulp(sc, i, j):
    sc["dtau_og"][i, j] = np.nextafter(sc["dtau"][i, j], np.inf)


NEAR = {"ftau_cld_tiny": _tiny_cloud, "ftau_ray_one_ulp": _ray_below_one, "w0_og_one_ulp": _w0_og_ulp,
        "dtau_og_one_ulp": _dtau_og_ulp}


@pytest.mark.parametrize("col", [0, NWNO - 1], ids=["first_column", "last_column"])      # the last sits in the partial wave
@pytest.mark.parametrize("layer", [0, 2])                                                # peeled first layer, interior
@pytest.mark.parametrize("name", list(NEAR))
def test_a_near_miss_in_one_column_unflags_the_layer(monkeypatch, ctx, name, layer, col):
    from picaso_amd import resident
    sc = _scene(6, [4])
    NEAR[name](sc, layer, col)
    _resum(sc)
    want = [i not in (layer, 4) for i in range(6)]
    assert np.array_equal(_np_mask(sc), want)
    d, _ = _check(monkeypatch, ctx, sc)
    assert resident.seal_reflected_planes(ctx, 7, NWNO, d) == 7          # the mask is no flag


@pytest.mark.parametrize("layer", [0, 2, 5])
def test_minus_zero_in_ftau_cld(monkeypatch, ctx, layer):
    """``-0.0 == 0.0``: the layer counts as clear, as it does for the kernel's own test, and the bits stay."""
    sc = _scene(6, [3])
    sc["ftau_cld"][layer, ::7] = -0.0
    sc["ftau_cld"][layer, NWNO - 1] = -0.0
    _check(monkeypatch, ctx, sc)


# ------------------------------------------------------------------------------------------------------------------------
# 6. invalidation
# ------------------------------------------------------------------------------------------------------------------------
def test_a_copy_that_puts_a_cloud_into_a_clear_layer_drops_the_mask_with_the_seal(monkeypatch, ctx):
    from picaso_amd import _lib, resident
    sc = _scene(6, [3])
    d, before = _check(monkeypatch, ctx, sc)
    n1 = resident.reflected_seal_stat(ctx)[0]
    sc2 = _scene(6, [2, 3])
    first = True
    for k in ("ftau_cld",) + tuple(p for p in resident.REFLECTED_PLANES if p != "ftau_cld"):
        a = np.ascontiguousarray(sc2[k])
        _lib.check(_lib.load().picaso_memcpy_h2d(ctx, d[k].addr, _lib.ptr(a), a.nbytes), ctx)
        if first:
            assert resident.reflected_seal_stat(ctx)[0] == n1 - 1
            assert resident.reflected_seal_layers(ctx, d["ftau_cld"]) is None
            first = False
    masks, hits, out = _abc(monkeypatch, ctx, lambda: _solve(ctx, d))
    assert (masks, hits) == (0, 0)
    assert not np.array_equal(out[1], before[1])
    fresh = resident.upload_scene(sc2, _keys(), ctx=ctx, seal=False)
    assert _same(out, _solve(ctx, fresh))


# ------------------------------------------------------------------------------------------------------------------------
# 7. batches
# ------------------------------------------------------------------------------------------------------------------------
def test_batch_of_sets_with_different_masks(monkeypatch, ctx):
    from picaso_amd import resident
    sets = [resident.upload_scene(_scene(6, cloudy, seed=seed), _keys(), ctx=ctx)
            for cloudy, seed in (([1], 31), ([4], 32), ([], 33))]
    masks, hits, out = _abc(monkeypatch, ctx, lambda: _solve_batch(ctx, sets))
    assert (masks, hits) == (1, 1)
    for s, d in enumerate(sets):
        m, _, own = _abc(monkeypatch, ctx, lambda: _solve(ctx, d))
        assert m == 1
        assert _same([out[s], out[3 + s]], own)


def test_batch_with_an_unsealed_member_runs_as_before(monkeypatch, ctx):
    from picaso_amd import resident
    sets = [resident.upload_scene(_scene(6, [1], seed=31), _keys(), ctx=ctx),
            resident.upload_scene(_scene(6, [4], seed=32), _keys(), ctx=ctx, seal=False)]
    masks, hits, _ = _abc(monkeypatch, ctx, lambda: _solve_batch(ctx, sets))
    assert (masks, hits) == (0, 0)


# ------------------------------------------------------------------------------------------------------------------------
# 8. a wavelength shard carries the mask of its own columns
# ------------------------------------------------------------------------------------------------------------------------
def test_a_sharded_upload_has_the_mask_of_its_own_columns(monkeypatch, ctx):
    comps = _components(6, [3])
    _cloud_row(comps, 1, slice(0, 40), np.random.default_rng(5))          # layer 1: cloud in columns [0, 40) only
    sc = _mix(comps)
    lo, hi = 40, NWNO - 3                                                  # 557 columns at a pitch of 557 doubles
    assert np.array_equal(_np_mask(sc), [True, False, True, False, True, True])
    assert np.array_equal(_np_mask(sc, lo, hi), [True, True, True, False, True, True])
    _, shard = _check(monkeypatch, ctx, sc, lo=lo, hi=hi)
    _, whole = _check(monkeypatch, ctx, sc)
    assert np.array_equal(shard[1], whole[1][lo:hi])
    assert np.array_equal(shard[0], whole[0][..., lo:hi])
