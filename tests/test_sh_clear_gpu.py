"""get_reflected_SH (reference fluxes.py:2675-2976, 3336-3607) for cloud-free columns with the angle-independent half of
each layer shared between the disk angles of a lane (`k_sh4_clear<NA>`, sh_clear.hip): the call with `dtau` and `w0` only
against the oracle on the full plane set, against the full-plane kernel (`k_sh`: to the oracle's tolerance, not bit for bit --
see the kernel's header), and the same bits however many angles share a lane and however the wavelengths are cut."""
import numpy as np
import pytest

from helpers import rel_err

pytestmark = pytest.mark.gpu

TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)               # frac_a, frac_b, frac_c, constant_back, constant_forward
OPTS = (0, 0, 0, 1, 1, 1)                        # the reference's default SH forms (config.json)
PLANES = ("dtau", "tau", "w0", "cosb", "ftau_cld", "ftau_ray", "f_deltaM", "dtau_og", "tau_og", "w0_og", "cosb_og")


@pytest.fixture(scope="module")
def hip():
    from picaso_amd import _lib, disco, fluxes
    assert _lib.device_count() > 0, "no MI355X visible"
    _lib.context()

    class H:
        pass
    h = H()
    h.fluxes, h.disco = fluxes, disco
    return h


def _geom(hip, ng, nt, phase):
    if nt == 1:
        g, gw, t, tw = hip.disco.get_angles_1d(ng)
    else:
        g, gw, t, tw = hip.disco.get_angles_3d(ng, nt)
    u0, u1, ct, _, _ = hip.disco.compute_disco(ng, nt, g, t, phase)
    return u0, u1, ct


def _scene(nlayer, nwno, seed, **kw):
    from picaso_amd import synthetic as syn
    sc = syn.make_scene(nlayer, nwno, seed=seed, stream=4, cloud=False, **kw)
    # what the reference's compute_opacity leaves for a cloud-free atmosphere (optics.py:303-431)
    assert not sc["ftau_cld"].any() and np.all(sc["ftau_ray"] == 1.0) and not sc["cosb_og"].any()
    assert not sc["f_deltaM"].any() and np.array_equal(sc["dtau"], sc["dtau_og"]) and np.array_equal(sc["w0"], sc["w0_og"])
    assert np.array_equal(sc["tau"], sc["tau_og"])
    return sc


def _call(fn, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, lean, b_top=0.0, lo=None, hi=None):
    cut = (lambda a: a) if lo is None else (lambda a: np.ascontiguousarray(a[..., lo:hi]))
    planes = [cut(sc[k]) if (not lean or k in ("dtau", "w0")) else None for k in PLANES]
    if not lean:
        planes[6] = planes[6].copy()                                  # f_deltaM is compounded in place
    n = nwno if lo is None else hi - lo
    rs_, f0_ = (cut(np.zeros(nwno) + rs), cut(np.zeros(nwno) + f0))
    x, _ = fn(nlayer + 1, n, ng, nt, *planes, rs_, u0, u1, ct, f0_, *OPTS, *TTHG, 4, b_top)
    return x


@pytest.mark.parametrize("ng,nt,phase", [(5, 1, 0.0), (8, 1, 0.0), (3, 2, 0.9), (4, 3, 2.1), (6, 1, 0.0), (7, 5, 1.2)])
def test_against_oracle_and_full_plane_kernel(hip, oracle, monkeypatch, ng, nt, phase):
    nlayer, nwno = 31, 523
    monkeypatch.delenv("PICASO_AMD_SHC_ANGLES", raising=False)
    rng = np.random.default_rng(17 * ng + nt)
    u0, u1, ct = _geom(hip, ng, nt, phase)
    for trial in range(3):
        sc = _scene(nlayer, nwno, 900 + 5 * trial + ng)
        rs = 0.4 * rng.random(nwno) if trial else 0.0
        f0 = 1.0 + rng.random(nwno) if trial == 2 else 1.0
        b_top = 0.0 if trial < 2 else 0.3
        got = _call(hip.fluxes.get_reflected_SH, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, True, b_top)
        want = _call(oracle.get_reflected_SH, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, False, b_top)
        assert rel_err(got, want) < 1e-9, (trial, "oracle")
        full = _call(hip.fluxes.get_reflected_SH, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, False, b_top)
        assert rel_err(got, full) < 1e-9, (trial, "full-plane kernel")
        for m in (1, 2):                                              # angles per lane: same bits
            monkeypatch.setenv("PICASO_AMD_SHC_ANGLES", str(m))
            alt = _call(hip.fluxes.get_reflected_SH, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, True, b_top)
            assert np.array_equal(alt, got), (trial, m)
        monkeypatch.delenv("PICASO_AMD_SHC_ANGLES")
        lo, hi = 130, 387                                             # a wavelength block alone: same bits
        part = _call(hip.fluxes.get_reflected_SH, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, True, b_top, lo, hi)
        assert np.array_equal(part, got[..., lo:hi]), trial


def test_thick_thin_conservative_and_single_layer(hip, oracle):
    """Layers far beyond the 35-clips, nearly transparent columns, w0 -> 1 and nlayer = 1."""
    u0, u1, ct = _geom(hip, 5, 1, 0.0)
    for nlayer, nwno, kw in ((40, 301, dict(gas_scale=300.0, ray_scale=30.0)), (40, 301, dict(gas_scale=1e-4, ray_scale=1e-3)),
                             (25, 200, dict(gas_scale=1e-7, ray_scale=5.0)), (1, 67, {}), (90, 129, dict(ray_scale=200.0))):
        sc = _scene(nlayer, nwno, 31 + nlayer, **kw)
        got = _call(hip.fluxes.get_reflected_SH, sc, nlayer, nwno, 5, 1, u0, u1, ct, 0.2, 1.0, True)
        want = _call(oracle.get_reflected_SH, sc, nlayer, nwno, 5, 1, u0, u1, ct, 0.2, 1.0, False)
        assert np.isfinite(got).all()
        assert rel_err(got, want, floor=1e-30) < 1e-9, (nlayer, kw)


def test_refusals(hip):
    """Some of the planes left out, stream 2, non-default forms, flx = 1: clean errors, not a wrong kernel."""
    from picaso_amd._lib import PicasoHipError
    from picaso_amd import resident
    nlayer, nwno = 9, 70
    sc = _scene(nlayer, nwno, 5)
    u0, u1, ct = _geom(hip, 5, 1, 0.0)
    head = (nlayer + 1, nwno, 5, 1)
    tail = (0.0, u0, u1, ct, 1.0)
    lean = [sc[k] if k in ("dtau", "w0") else None for k in PLANES]
    partial = list(lean)
    partial[1] = sc["tau"]
    with pytest.raises(PicasoHipError, match="all of"):
        hip.fluxes.get_reflected_SH(*head, *partial, *tail, *OPTS, *TTHG, 4)
    with pytest.raises(PicasoHipError, match="stream 4"):
        hip.fluxes.get_reflected_SH(*head, *lean, *tail, *OPTS, *TTHG, 2)
    with pytest.raises(PicasoHipError, match="stream 4"):
        hip.fluxes.get_reflected_SH(*head, *lean, *tail, 1, 0, 0, 1, 1, 1, *TTHG, 4)
    with pytest.raises(PicasoHipError, match="stream 4"):
        hip.fluxes.get_reflected_SH(*head, *lean, *tail, *OPTS, *TTHG, 4, 0.0, 1)
    assert resident.reflected_SH_can_derive(4) and not resident.reflected_SH_can_derive(2)
    assert not resident.reflected_SH_can_derive(4, w_multi_form=1) and not resident.reflected_SH_can_derive(4, flx=1)


# ---- a cloud-free TOP above a cloud deck: picaso_get_reflected_SH_top_dev (cloud_free_above) ----

def _resident_call(hip, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, top, lo=None, hi=None):
    from picaso_amd import _lib, device, resident
    ctx = _lib.context()
    scn = dict(sc)
    scn["F0PI"] = np.zeros(nwno) + f0
    scn["surf_reflect"] = np.zeros(nwno) + rs
    d = resident.upload_scene(scn, resident.SH_PLANES + ("F0PI", "surf_reflect"), lo, hi, ctx=ctx)
    n = nwno if lo is None else hi - lo
    x = device.DeviceArray((ng, nt, n), ctx)
    resident.reflected_SH(ctx, nlayer + 1, n, ng, nt, d, d["surf_reflect"], u0, u1, ct, d["F0PI"], *OPTS, *TTHG, 4, x,
                          cloud_free_above=top)
    return x.to_host()


@pytest.mark.parametrize("ng,nt,phase", [(5, 1, 0.0), (4, 3, 1.4), (7, 3, 0.6)])
def test_cloud_free_top_above_a_cloud_deck(hip, oracle, monkeypatch, ng, nt, phase):
    """The layers above the cloud slab through k_sh4_clear, the rest through k_sh from the state it leaves: against the
    oracle and the unsplit launch (1e-9), the same bits for a wavelength block alone and at either number of angles per
    lane; cloud_free_above = 0 (and < 4) IS the unsplit launch."""
    from picaso_amd import synthetic as syn
    nlayer, nwno = 40, 389
    monkeypatch.setenv("PICASO_AMD_SH_CHECK_TOP", "1")
    u0, u1, ct = _geom(hip, ng, nt, phase)
    rng = np.random.default_rng(5 + ng)
    for trial in range(2):
        sc = syn.make_scene(nlayer, nwno, seed=700 + trial + ng, stream=4)
        deck = int(np.argmax(sc["ftau_cld"].any(axis=1)))             # first cloudy layer (0.55 nlayer = 22)
        assert deck == 22 and not sc["cosb_og"][:deck].any()
        rs = 0.3 * rng.random(nwno) if trial else 0.0
        f0 = 1.0 + rng.random(nwno)
        planes = [np.array(sc[k]) for k in PLANES]
        want, _ = oracle.get_reflected_SH(nlayer + 1, nwno, ng, nt, *planes, np.zeros(nwno) + rs, u0, u1, ct, f0, *OPTS,
                                          *TTHG, 4)
        plain = _resident_call(hip, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, 0)
        assert rel_err(plain, want) < 1e-9
        for top in (deck, 10, 4):
            got = _resident_call(hip, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, top)
            assert rel_err(got, want) < 1e-9, (trial, top, "oracle")
            assert rel_err(got, plain) < 1e-9 and not np.array_equal(got, plain), (trial, top)
            part = _resident_call(hip, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, top, 101, 300)
            assert np.array_equal(part, got[..., 101:300]), (trial, top, "block")
            for m in (1, 2):
                monkeypatch.setenv("PICASO_AMD_SHC_ANGLES", str(m))
                assert np.array_equal(_resident_call(hip, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, top), got), (top, m)
            monkeypatch.delenv("PICASO_AMD_SHC_ANGLES")
        assert np.array_equal(_resident_call(hip, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, 3), plain)
        monkeypatch.setenv("PICASO_AMD_SH_NO_TOP", "1")
        assert np.array_equal(_resident_call(hip, sc, nlayer, nwno, ng, nt, u0, u1, ct, rs, f0, deck), plain)
        monkeypatch.delenv("PICASO_AMD_SH_NO_TOP")


def test_cloud_free_top_statement_is_checked_on_request(hip, monkeypatch):
    """A cloud_free_above that reaches into the cloud: PICASO_AMD_SH_CHECK_TOP=1 fails the call; the whole column
    (cloud_free_above >= nlayer on a cloud-free scene) is the cloud-free form's bits."""
    from picaso_amd import synthetic as syn
    from picaso_amd._lib import PicasoHipError
    nlayer, nwno = 20, 130
    u0, u1, ct = _geom(hip, 5, 1, 0.0)
    sc = syn.make_scene(nlayer, nwno, seed=11, stream=4)
    monkeypatch.setenv("PICASO_AMD_SH_CHECK_TOP", "1")
    with pytest.raises(PicasoHipError, match="cloud_free_above = 12"):
        _resident_call(hip, sc, nlayer, nwno, 5, 1, u0, u1, ct, 0.0, 1.0, 12)           # the slab starts at layer 11
    _resident_call(hip, sc, nlayer, nwno, 5, 1, u0, u1, ct, 0.0, 1.0, 11)
    clear = _scene(nlayer, nwno, 12)
    whole = _resident_call(hip, clear, nlayer, nwno, 5, 1, u0, u1, ct, 0.1, 1.0, nlayer + 5)
    lean = _call(hip.fluxes.get_reflected_SH, clear, nlayer, nwno, 5, 1, u0, u1, ct, 0.1, 1.0, True)
    assert np.array_equal(whole, lean)


@pytest.mark.parametrize("stream", [2, 4])
@pytest.mark.parametrize("phase", [0.0, 1.1])
def test_sh_level_planes_left_out_running_products(stream, phase):
    """tau and tau_og left out (picaso_reflected_SH_can_derive_levels): the launch carries exp(-tau/u0) and
    exp(-tau_og/u0) as running products of the layers' exp(-dtau/u0) (in the symmetric geometry the exp(-dtau/u1) at hand)
    instead of reading the planes and forming two more exponentials per layer.  Against the plane-reading launch: the
    rounding of the products times the conditioning of the layer systems (observed <= 5e-12, SH2 at the larger end), for
    thin and for 35-clipped thick columns, with and without the cloud-free top split; a column's bits do not depend on the wavelength block it is launched in."""
    from picaso_amd import _lib, device, disco, resident
    from picaso_amd import synthetic as syn
    ctx = _lib.context()
    nlayer, nwno = 41, 777
    if phase == 0.0:
        g, gw, t, tw = disco.get_angles_1d(5)
        nt = 1
    else:
        g, gw, t, tw = disco.get_angles_3d(3, 2)
        nt = 2
    u0, u1, cth, _, _ = disco.compute_disco(len(g), nt, g, t, phase)
    ct = 1.0 if phase == 0.0 else float(cth)
    ng = len(g)
    opts = (0, 0, 0, 1, 1, 1, 1.0, -1.0, 2.0, -0.5, 1.0, stream)
    assert resident.reflected_SH_can_derive_levels(nlayer + 1, nwno, stream)
    assert not resident.reflected_SH_can_derive_levels(nlayer + 1, nwno, stream, w_single_form=1)
    for seed, kw in ((3, {}), (4, dict(gas_scale=80.0, cloud_opd=30.0)), (5, dict(cloud=False))):
        sc = syn.make_scene(nlayer, nwno, seed=seed, stream=stream, **kw)
        sc["F0PI"] = np.linspace(0.8, 1.2, nwno)
        sc["surf_reflect"] = np.full(nwno, 0.2)
        d = resident.upload_scene(sc, resident.SH_PLANES + ("F0PI", "surf_reflect"), ctx=ctx)
        lean = {k: v for k, v in d.items() if k not in ("tau", "tau_og")}

        def run(planes, top=0, lo=0, hi=nwno):
            n = hi - lo
            pl = planes if (lo, hi) == (0, nwno) else {k: device.DeviceArray.from_host(
                np.ascontiguousarray(sc[k][:, lo:hi]), ctx) for k in planes if k in resident.SH_PLANES}
            rs = device.DeviceArray.from_host(sc["surf_reflect"][lo:hi], ctx)
            f0 = device.DeviceArray.from_host(sc["F0PI"][lo:hi], ctx)
            x = device.DeviceArray((ng, nt, n), ctx)
            resident.reflected_SH(ctx, nlayer + 1, n, ng, nt, pl, rs, u0, u1, ct, f0, *opts, x, cloud_free_above=top)
            return x.to_host()
        full, drv = run(d), run(lean)
        assert np.isfinite(drv).all()
        assert np.max(np.abs(drv - full) / np.abs(full)) < 1e-10, (seed, stream, phase)
        # launch-shape invariance of the derived form
        part = run(lean, lo=100, hi=400)
        assert np.array_equal(part, drv[:, :, 100:400])
        if stream == 4 and seed == 3:
            from picaso_amd import justdoit as jdi           # noqa: F401
            top = int(np.argmax((sc["ftau_cld"] != 0).any(axis=1)))
            if top >= 4:
                a, b = run(d, top=top), run(lean, top=top)
                assert np.max(np.abs(b - a) / np.abs(a)) < 1e-10
                assert np.max(np.abs(b - full) / np.abs(full)) < 1e-9
    # options outside the default set: the launch asks for the planes
    with pytest.raises(Exception, match="tau and tau_og may be left out"):
        x = device.DeviceArray((ng, nt, nwno), ctx)
        resident.reflected_SH(ctx, nlayer + 1, nwno, ng, nt, lean, d["surf_reflect"], u0, u1, ct, d["F0PI"], 1, 1, 1, 1, 1, 1,
                              1.0, -1.0, 2.0, -0.5, 1.0, stream, x)
