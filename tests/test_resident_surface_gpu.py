"""The keyword surface the spectrum path uses on ``resident``: ``reflected_1d(lvl_fluxes=)``, ``reflected_SH(flux=)`` and
``thermal_SH``, each bit for bit against the host entry of ``fluxes.py`` on the same arrays -- the host entry is an upload
plus the same ``*_dev`` call.  11 levels, 130 columns (two full waves and a two-lane tail), a cloudy synthetic scene."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NLEVEL, NWNO = 11, 130
TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)
DISKS = {"1x1": (1, 1), "3x2": (3, 2)}


def _scene(stream):
    from picaso_amd import synthetic as syn
    sc = syn.make_scene(NLEVEL - 1, NWNO, seed=31, stream=stream)
    sc["F0PI"] = np.linspace(0.8, 1.3, NWNO)
    sc["surf_reflect"] = np.linspace(0.05, 0.3, NWNO)
    return sc


def _disk(ng, nt):
    u0 = np.linspace(0.95, 0.25, ng * nt).reshape(ng, nt)
    return u0, np.ascontiguousarray(u0[::-1, ::-1]) * 0.9 + 0.05, 0.8


@pytest.mark.parametrize("disk", list(DISKS))
def test_reflected_1d_level_fluxes_equal_the_host_entry(disk):
    from picaso_amd import _lib, fluxes, resident
    from picaso_amd.device import DeviceArray
    (ng, nt), ctx, sc = DISKS[disk], _lib.context(), _scene(2)
    u0, u1, ct = _disk(ng, nt)
    want_x, want_lvl = fluxes.get_reflected_1d(NLEVEL, sc["wno"], NWNO, ng, nt, *[sc[k] for k in resident.REFLECTED_PLANES],
                                               sc["surf_reflect"], u0, u1, ct, sc["F0PI"], 3, 0, *TTHG, get_lvl_flux=1)
    d = resident.upload_scene(sc, resident.REFLECTED_PLANES + ("F0PI", "surf_reflect"), ctx=ctx, seal=False)
    x = DeviceArray((ng, nt, NWNO), ctx)
    lvl = [DeviceArray((ng, nt, NLEVEL, NWNO), ctx) for _ in range(4)]
    resident.reflected_1d(ctx, NLEVEL, NWNO, ng, nt, d, d["surf_reflect"], u0, u1, ct, d["F0PI"], 3, 0, *TTHG, x,
                          lvl_fluxes=lvl)
    assert np.array_equal(x.to_host(), want_x)
    for got, want in zip(lvl, want_lvl):
        assert np.any(want != 0) and np.array_equal(got.to_host(), want)


@pytest.mark.parametrize("stream", [2, 4])
@pytest.mark.parametrize("disk", list(DISKS))
def test_reflected_SH_layer_fluxes_equal_the_host_entry(disk, stream):
    from picaso_amd import _lib, fluxes, resident
    from picaso_amd.device import DeviceArray
    (ng, nt), ctx, sc = DISKS[disk], _lib.context(), _scene(stream)
    u0, u1, ct = _disk(ng, nt)
    opts = (0, 0, 0, 1, 1, 1, *TTHG, stream)
    d = resident.upload_scene(sc, resident.SH_PLANES + ("F0PI", "surf_reflect"), ctx=ctx)
    # (the host entry leaves the caller's f_deltaM compounded, as the reference does: it gets copies)
    want_x, want_flux = fluxes.get_reflected_SH(NLEVEL, NWNO, ng, nt, *[sc[k].copy() for k in resident.SH_PLANES],
                                                sc["surf_reflect"], u0, u1, ct, sc["F0PI"], *opts, flx=1)
    x, flux = DeviceArray((ng, nt, NWNO), ctx), DeviceArray((ng, nt, stream * NLEVEL, NWNO), ctx)
    resident.reflected_SH(ctx, NLEVEL, NWNO, ng, nt, d, d["surf_reflect"], u0, u1, ct, d["F0PI"], *opts, x, flux=flux)
    assert np.array_equal(x.to_host(), want_x)
    assert np.any(want_flux != 0) and np.array_equal(flux.to_host(), want_flux)


@pytest.mark.parametrize("stream", [2, 4])
@pytest.mark.parametrize("disk", list(DISKS))
def test_thermal_SH_equals_the_host_entry(disk, stream):
    from picaso_amd import _lib, fluxes, resident
    from picaso_amd.device import DeviceArray
    (ng, nt), ctx, sc = DISKS[disk], _lib.context(), _scene(stream)
    _, u1, _ = _disk(ng, nt)
    want, _ = fluxes.get_thermal_SH(NLEVEL, sc["wno"], NWNO, ng, nt, sc["tlevel"], sc["dtau"], sc["tau"], sc["w0"], sc["cosb"],
                                    sc["dtau_og"], sc["tau_og"], sc["w0_og"], sc["w0_no_raman"], sc["cosb_og"], sc["plevel"],
                                    u1, sc["surf_reflect"], stream, 1)
    differs = not np.array_equal(sc["cosb"], sc["cosb_og"])        # the host entry's own test (fluxes.py:3072)
    assert differs
    d = resident.upload_scene(sc, ("wno", "dtau", "tau", "w0", "cosb_og", "surf_reflect"), ctx=ctx)
    x = DeviceArray((ng, nt, NWNO), ctx)
    resident.thermal_SH(ctx, NLEVEL, d["wno"], NWNO, ng, nt, sc["tlevel"], d["dtau"], d["w0"], d["cosb_og"], sc["plevel"], u1,
                        d["surf_reflect"], stream, 1, differs, x, tau=d["tau"])
    assert np.all(np.isfinite(want)) and np.array_equal(x.to_host(), want)
