"""Every launch wrapper of ``picaso_amd.resident`` hands each of its arguments to the header parameter of that name.

No GPU and no library: ``resident.load`` is replaced by a recorder, the device arrays by stand-ins with distinct
addresses, and the recorded positional arguments are compared, parameter name by parameter name, with the prototypes of
``include/picaso_hip.h`` (which names every parameter).  A case lists the wrapper's arguments in the wrapper's own order
(that order and the names are public: ``bench.py``, ``tools/`` and the tests call positionally) and, for EVERY parameter
of the C function, the value it must receive.
"""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

from picaso_amd import _lib, resident
from picaso_amd.planes import REFLECTED_PLANES, SH_PLANES

PARAMS = _lib.declared_parameters()
NLEVEL, NWNO, NG, NT, NGAUSS, NSPEC = 7, 13, 3, 2, 4, 3
NFAC = NG * NT
CTX = object()
_next = itertools.count(1)


class Dev:
    """Stand-in for a DeviceArray: an address of its own, never dereferenced."""

    def __init__(self, *shape):
        self.addr = next(_next) << 24
        self.shape = shape
        self.nbytes = 8 * int(np.prod(shape))


class Recorder:
    """What ``resident.load()`` returns here: every ``picaso_*`` is a callable that stores its arguments and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("picaso_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))      # holding the arguments keeps the host arrays behind the pointers alive
            return 0
        return call


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(resident, "load", lambda: r)
    return r


def _address(arg):
    if arg is None or isinstance(arg, int):
        return arg
    if not isinstance(arg, ctypes._Pointer):
        return NotImplemented                              # a float, a table, ...: not an address
    return ctypes.cast(arg, ctypes.c_void_p).value


def _matches(arg, exp):
    if exp is CTX:
        return arg is CTX
    if exp is None:
        return arg is None
    if isinstance(exp, Dev):
        return _address(arg) == exp.addr
    if isinstance(exp, np.ndarray):                        # a host array: by content
        if not isinstance(arg, _lib.c_double_p):
            return False
        return np.array_equal(np.ctypeslib.as_array(arg, shape=(exp.size,)), exp.ravel())
    if isinstance(exp, list):                              # a pointer table: by entries
        if not isinstance(arg, ctypes.Array) or len(arg) != max(1, len(exp)):
            return False
        return [arg[i] for i in range(len(exp))] == [getattr(e, "addr", e) for e in exp]
    return isinstance(arg, (int, float)) and not isinstance(arg, bool) and arg == exp


def _call(fn, kw):
    """``fn`` with the arguments ``kw``: those without a default positionally, in ``kw``'s order, which must be the
    signature's."""
    sig = inspect.signature(fn).parameters
    assert set(kw) <= set(sig), "%s: parameter names changed" % fn.__name__
    required = [p for p, v in sig.items() if v.default is inspect.Parameter.empty]
    assert required == list(kw)[:len(required)], "%s: required parameters changed" % fn.__name__
    fn(*[kw[p] for p in required], **{p: v for p, v in kw.items() if p not in required})


def _verify(call, func, spec):
    name, args = call
    names = PARAMS[func]
    assert name == func
    assert len(args) == len(names)
    assert sorted(spec) == sorted(names), "the case must pin every parameter of %s" % func
    wrong = [n for n, a in zip(names, args) if not _matches(a, spec[n])]
    assert not wrong, "%s: wrong value at parameter(s) %s" % (func, wrong)


# ---------------------------------------------------------------------------------------------- shared stand-ins
U0 = 0.1 + np.arange(NFAC, dtype=float).reshape(NG, NT) / 10
U1 = U0 + 0.03
U0S = np.stack([U0 + 0.001 * s for s in range(NSPEC)])
U1S = np.stack([U1 + 0.001 * s for s in range(NSPEC)])
CTS = np.array([0.71, 0.72, 0.73])
GW, TW = np.array([0.2, 0.3, 0.5]), np.array([0.4, 0.6])
WTS = np.array([0.1, 0.2, 0.3, 0.4])
TL, PL = 500.0 + np.arange(NLEVEL), 1e-3 * (1 + np.arange(NLEVEL))
TLS, PLS = np.stack([TL + 10 * s for s in range(NSPEC)]), np.stack([PL * (s + 2) for s in range(NSPEC)])
TL3 = 300.0 + np.arange(NLEVEL * NFAC, dtype=float).reshape(NLEVEL, NG, NT)
PL3 = 2.0 * TL3
TL3S, PL3S = np.stack([TL3 + 1000 * s for s in range(NSPEC)]), np.stack([PL3 + 1000 * s for s in range(NSPEC)])
TTHG = dict(single_phase=3, multi_phase=1, frac_a=0.11, frac_b=0.22, frac_c=0.33, constant_back=0.44,
            constant_forward=0.55)
FORMS = dict(w_single_form=2, w_multi_form=3, psingle_form=4, w_single_rayleigh=5, w_multi_rayleigh=6,
             psingle_rayleigh=7)
NONE4 = dict.fromkeys(("flux_minus_all", "flux_plus_all", "flux_minus_midpt_all", "flux_plus_midpt_all"))
TNONE4 = dict.fromkeys(("flux_minus", "flux_plus", "flux_minus_mdpt", "flux_plus_mdpt"))


def _planes(names, skip=()):
    return {k: Dev(NLEVEL, NWNO) for k in names if k not in skip}


def _columns(names, planes, suffix=""):
    """Header parameter -> what a list of plane dictionaries puts there (a family left out of all: NULL)."""
    return {k + suffix: ([pl[k] for pl in planes] if planes[0].get(k) is not None else None) for k in names}


def _devs(n, *shape):
    return [Dev(*shape) for _ in range(n)]


# ---------------------------------------------------------------------------------------------- the cases
def case_reflected_1d(weights=False, lvl=False):
    pl = _planes(REFLECTED_PLANES, skip=() if weights else ("tau", "gcos2"))
    rs, f0, x, alb = Dev(NWNO), Dev(NWNO), Dev(NG, NT, NWNO), Dev(NWNO)
    kw = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, numg=NG, numt=NT, planes=pl, surf_reflect=rs, ubar0=U0, ubar1=U1,
              cos_theta=0.7, F0PI=f0, **TTHG, xint_at_top=x)
    spec = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, plane_pitch=NWNO, numg=NG, numt=NT, **{k: pl.get(k) for k in REFLECTED_PLANES},
                surf_reflect=rs, ubar0=U0, ubar1=U1, cos_theta=0.7, F0PI=f0, **TTHG, get_toa_intensity=1, get_lvl_flux=0,
                toon_coefficients=0, b_top=0.0, xint_at_top=x, **NONE4, gweight=None, tweight=None, albedo=None)
    if weights:
        kw.update(toon_coefficients=1, b_top=0.66, gweight=GW, tweight=TW, albedo=alb, plane_pitch=NWNO + 3)
        spec.update(toon_coefficients=1, b_top=0.66, gweight=GW, tweight=TW, albedo=alb, plane_pitch=NWNO + 3)
    if lvl:
        lv = _devs(4, NG, NT, NLEVEL, NWNO)
        kw.update(lvl_fluxes=lv)
        spec.update(zip(NONE4, lv), get_lvl_flux=1)
    return resident.reflected_1d, kw, "picaso_get_reflected_1d_dev", spec


def case_thermal_1d(full=False):
    wno, dtau, w0, cosb, rs, fx = Dev(NWNO), Dev(1), Dev(1), Dev(1), Dev(NWNO), Dev(NG, NT, NWNO)
    kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, numg=NG, numt=NT, tlevel=TL, dtau=dtau, w0=w0, cosb=cosb, plevel=PL,
              ubar1=U1, surf_reflect=rs, hard_surface=1, flux_at_top=fx)
    spec = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, plane_pitch=NWNO, numg=NG, numt=NT, tlevel=TL, dtau=dtau, w0=w0,
                cosb=cosb, plevel=PL, ubar1=U1, surf_reflect=rs, hard_surface=1, dwno=None, calc_type=0, flux_at_top=fx,
                **TNONE4, gweight=None, tweight=None, flux_disk=None)
    if full:
        dwno, disk, lv = Dev(NWNO), Dev(NWNO), _devs(4, 1)
        opts = dict(dwno=dwno, calc_type=1, gweight=GW, tweight=TW, flux_disk=disk, plane_pitch=NWNO + 5)
        kw.update(opts, lvl_fluxes=lv)
        spec.update(opts)
        spec.update(zip(TNONE4, lv))
    return resident.thermal_1d, kw, "picaso_get_thermal_1d_dev", spec


def _geometry(per_spectrum):
    if per_spectrum:
        return dict(ubar0=U0S, ubar1=U1S, cos_theta=CTS), NSPEC
    return dict(ubar0=U0, ubar1=U1, cos_theta=0.7), 1


def _reflected_batch(fn, func, names, options, per_spectrum, fuse, defaults, extra=None, skip=()):
    pls = [_planes(names, skip) for _ in range(NSPEC)]
    rs, f0s, xs, albs = Dev(NWNO), _devs(NSPEC, NWNO), _devs(NSPEC, 1), _devs(NSPEC, NWNO)
    geo, ngeom = _geometry(per_spectrum)
    kw = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, numg=NG, numt=NT, planes=pls, surf_reflect=rs, **geo, F0PI=f0s, **options,
              xint_at_top=xs)
    # weights without an albedo, or an albedo without weights: nothing of the disk sum is handed over
    kw.update(dict(gweight=GW, tweight=TW, albedo=albs) if fuse else dict(gweight=GW, albedo=albs))
    kw.update(extra or {})
    spec = dict(ctx=CTX, nspec=NSPEC, nlevel=NLEVEL, nwno=NWNO, numg=NG, numt=NT, surf_reflect=[rs] * NSPEC,
                ubar0=geo["ubar0"], ubar1=geo["ubar1"], cos_theta=np.zeros(ngeom) + geo["cos_theta"], F0PI=f0s, **options,
                xint_at_top=xs, gweight=GW if fuse else None, tweight=TW if fuse else None, albedo=albs if fuse else None)
    spec.update(defaults)
    spec.update(extra or {})
    return fn, kw, func, spec, pls, ngeom


def case_reflected_1d_batch(per_spectrum, fuse):
    extra = dict(toon_coefficients=1, b_top=0.66, plane_pitch=NWNO + 3) if fuse else None
    fn, kw, func, spec, pls, ngeom = _reflected_batch(
        resident.reflected_1d_batch, "picaso_get_reflected_1d_batch_dev", REFLECTED_PLANES, TTHG, per_spectrum, fuse,
        dict(toon_coefficients=0, b_top=0.0, plane_pitch=NWNO), extra, skip=("gcos2",))
    spec.update(_columns(REFLECTED_PLANES, pls), ngeom=ngeom)
    spec["gcos2"] = [None] * NSPEC              # a table of NULLs, not a NULL table: this entry takes a plane per spectrum
    return fn, kw, func, spec


def case_reflected_SH_batch(per_spectrum, fuse):
    extra = dict(b_top=0.66, single_form=1, compound_f_deltaM=False, plane_pitch=NWNO + 3) if fuse else None
    fn, kw, func, spec, pls, ngeom = _reflected_batch(
        resident.reflected_SH_batch, "picaso_get_reflected_SH_batch_dev", SH_PLANES,
        dict(FORMS, **{k: v for k, v in TTHG.items() if "phase" not in k}, stream=4), per_spectrum, fuse,
        dict(b_top=0.0, single_form=0, compound_f_deltaM=1, plane_pitch=NWNO), extra)
    spec.update(_columns(SH_PLANES, pls), ngeom=ngeom)
    if fuse:
        spec["compound_f_deltaM"] = 0
    return fn, kw, func, spec


def case_reflected_3d_batch(fuse):
    fn, kw, func, spec, pls, _ = _reflected_batch(
        resident.reflected_3d_batch, "picaso_get_reflected_3d_batch_dev", REFLECTED_PLANES, TTHG, True, fuse, {},
        skip=("tau", "tau_og", "gcos2"))
    for k in ("ubar0", "ubar1", "cos_theta", "surf_reflect", "F0PI", "xint_at_top", "gweight", "tweight", "albedo"):
        assert k in spec
    spec.update(_columns(REFLECTED_PLANES, pls, "_3d"))
    return fn, kw, func, spec


def case_thermal_1d_batch(per_spectrum, fuse):
    wno, dwno, rs = Dev(NWNO), Dev(NWNO), Dev(NWNO)
    dtau, w0, cosb, fx, disk = (_devs(NSPEC, 1) for _ in range(5))
    u1 = U1S if per_spectrum else U1
    kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, numg=NG, numt=NT, tlevel=TLS, dtau=dtau, w0=w0, cosb=cosb, plevel=PL,
              ubar1=u1, surf_reflect=rs, hard_surface=True, flux_at_top=fx)
    kw.update(dict(dwno=dwno, calc_type=1, gweight=GW, tweight=TW, flux_disk=disk, plane_pitch=NWNO + 5) if fuse
              else dict(tweight=TW, flux_disk=disk))
    spec = dict(ctx=CTX, nspec=NSPEC, nlevel=NLEVEL, wno=wno, nwno=NWNO, plane_pitch=NWNO + 5 if fuse else NWNO, numg=NG,
                numt=NT, tlevel=TLS, dtau=dtau, w0=w0, cosb=cosb, plevel=np.broadcast_to(PL, (NSPEC, NLEVEL)),
                ngeom=NSPEC if per_spectrum else 1, ubar1=u1, surf_reflect=[rs] * NSPEC, hard_surface=1,
                dwno=dwno if fuse else None, calc_type=1 if fuse else 0, flux_at_top=fx, gweight=GW if fuse else None,
                tweight=TW if fuse else None, flux_disk=disk if fuse else None)
    return resident.thermal_1d_batch, kw, "picaso_get_thermal_1d_batch_dev", spec


def case_reflected_1d_ck(lvl):
    pl, rs, f0, x, alb = _planes(REFLECTED_PLANES), Dev(NWNO), Dev(NWNO), Dev(1), Dev(NWNO)
    kw = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, ngauss=NGAUSS, numg=NG, numt=NT, planes=pl, surf_reflect=rs, ubar0=U0, ubar1=U1,
              cos_theta=0.7, F0PI=f0, **TTHG, gauss_wts=WTS, xint_at_top=x)
    spec = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, ngauss=NGAUSS, numg=NG, numt=NT, **pl, surf_reflect=rs, ubar0=U0, ubar1=U1,
                cos_theta=0.7, F0PI=f0, **TTHG, get_toa_intensity=1, get_lvl_flux=0, toon_coefficients=0, b_top=0.0,
                gauss_wts=WTS, xint_at_top=x, **NONE4, gweight=None, tweight=None, albedo=None)
    if lvl:
        lv = _devs(4, 1)
        opts = dict(toon_coefficients=1, b_top=0.66, gweight=GW, tweight=TW, albedo=alb, get_toa_intensity=0)
        kw.update(opts, lvl_fluxes=lv)
        spec.update(opts, get_lvl_flux=1)
        spec.update(zip(NONE4, lv))
    return resident.reflected_1d_ck, kw, "picaso_get_reflected_1d_ck_dev", spec


def case_thermal_1d_ck(lvl):
    wno, dtau, w0, cosb, rs, fx = Dev(NWNO), Dev(1), Dev(1), Dev(1), Dev(NWNO), Dev(1)
    kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, ngauss=NGAUSS, numg=NG, numt=NT, tlevel=TL, dtau=dtau, w0=w0,
              cosb=cosb, plevel=PL, ubar1=U1, surf_reflect=rs, hard_surface=0, gauss_wts=WTS, flux_at_top=fx)
    spec = dict(kw, dwno=None, calc_type=0, **TNONE4, gweight=None, tweight=None, flux_disk=None)
    if lvl:
        lv = _devs(4, 1)
        opts = dict(dwno=Dev(NWNO), calc_type=1, gweight=GW, tweight=TW, flux_disk=Dev(NWNO))
        kw.update(opts, lvl_fluxes=lv)
        spec.update(opts)
        spec.update(zip(TNONE4, lv))
    return resident.thermal_1d_ck, kw, "picaso_get_thermal_1d_ck_dev", spec


def case_tbatch(nets):
    wno, dtau, w0, cosb, rs, dwno = Dev(NWNO), Dev(1), Dev(1), Dev(1), Dev(NWNO), Dev(NWNO)
    kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, ngauss=NGAUSS, numg=NG, numt=NT, tlevels=TLS, dtau=dtau, w0=w0,
              cosb=cosb, plevel=PL, ubar1=U1, surf_reflect=rs, hard_surface=1, gauss_wts=WTS, gweight=GW, tweight=TW)
    spec = dict(kw, nitem=NSPEC, tlevel=TLS, dwno=dwno)
    del spec["tlevels"]
    if nets:
        out = dict(net_layer=Dev(1), net=Dev(1))
        kw.update(dwno=dwno, **out)
        spec.update(out)
        return resident.thermal_nets_tbatch, kw, "picaso_thermal_nets_tbatch_dev", spec
    d4 = Dev(1)
    kw.update(disk4=d4, dwno=dwno, calc_type=1)
    spec.update(disk4=d4, calc_type=1)
    return resident.thermal_1d_ck_tbatch, kw, "picaso_get_thermal_1d_ck_tbatch_dev", spec


def _sh_options():
    return dict(FORMS, **{k: v for k, v in TTHG.items() if "phase" not in k}, stream=4)


def case_reflected_SH(full=False, flux=False):
    pl = _planes(SH_PLANES, skip=() if full else ("tau", "tau_og"))
    rs, f0, x, alb = Dev(NWNO), Dev(NWNO), Dev(1), Dev(NWNO)
    kw = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, numg=NG, numt=NT, planes=pl, surf_reflect=rs, ubar0=U0, ubar1=U1,
              cos_theta=0.7, F0PI=f0, **_sh_options(), xint_at_top=x)
    spec = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, plane_pitch=NWNO, numg=NG, numt=NT, **{k: pl.get(k) for k in SH_PLANES},
                surf_reflect=rs, ubar0=U0, ubar1=U1, cos_theta=0.7, F0PI=f0, **_sh_options(), b_top=0.0, flx=0, single_form=0,
                compound_f_deltaM=1, cloud_free_above=0, xint_at_top=x, flux=None, gweight=None, tweight=None, albedo=None)
    if full:
        opts = dict(b_top=0.66, single_form=1, gweight=GW, tweight=TW, albedo=alb, plane_pitch=NWNO + 3, cloud_free_above=2)
        kw.update(opts, compound_f_deltaM=False)
        spec.update(opts, compound_f_deltaM=0)
    if flux:
        fl = Dev(1)
        kw.update(flux=fl)
        spec.update(flux=fl, flx=1)
    return resident.reflected_SH, kw, "picaso_get_reflected_SH_top_dev", spec


def case_reflected_SH_ck(full):
    pl, rs, f0, x, alb = _planes(SH_PLANES), Dev(NWNO), Dev(NWNO), Dev(1), Dev(NWNO)
    kw = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, ngauss=NGAUSS, numg=NG, numt=NT, planes=pl, surf_reflect=rs, ubar0=U0, ubar1=U1,
              cos_theta=0.7, F0PI=f0, **_sh_options(), gauss_wts=WTS, xint_at_top=x)
    spec = dict(kw, **pl, b_top=0.0, single_form=0, compound_f_deltaM=1, cloud_free_above=0, gweight=None, tweight=None,
                albedo=None)
    del spec["planes"]
    if full:
        opts = dict(b_top=0.66, single_form=1, cloud_free_above=2, gweight=GW, tweight=TW, albedo=alb)
        kw.update(opts, compound_f_deltaM=False)
        spec.update(opts, compound_f_deltaM=0)
    return resident.reflected_SH_ck, kw, "picaso_get_reflected_SH_ck_dev", spec


def case_thermal_SH(ck, full):
    wno, dtau, w0, cosb, rs, x = Dev(NWNO), Dev(1), Dev(1), Dev(1), Dev(NWNO), Dev(1)
    kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, numg=NG, numt=NT, tlevel=TL, dtau=dtau, w0=w0, cosb_og=cosb, plevel=PL,
              ubar1=U1, surf_reflect=rs, stream=4, hard_surface=1, cosb_differs_from_cosb_og=True, xint_at_top=x)
    spec = dict(kw, cosb_differs_from_cosb_og=1, tau=None, gweight=None, tweight=None, flux_disk=None)
    if full:
        opts = dict(tau=Dev(1), gweight=GW, tweight=TW, flux_disk=Dev(NWNO))
        kw.update(opts, cosb_differs_from_cosb_og=0)
        spec.update(opts, cosb_differs_from_cosb_og=0)
    if ck:
        kw = {k: v for k, v in kw.items() if k not in ("numg", "numt", "xint_at_top")}
        kw = dict(list(kw.items())[:4] + [("ngauss", NGAUSS), ("numg", NG), ("numt", NT)] + list(kw.items())[4:])
        kw = dict(list(kw.items())[:17] + [("gauss_wts", WTS), ("xint_at_top", x)] + list(kw.items())[17:])
        spec.update(ngauss=NGAUSS, gauss_wts=WTS)
        return resident.thermal_SH_ck, kw, "picaso_get_thermal_SH_ck_dev", spec
    if full:
        kw.update(plane_pitch=NWNO + 3)
    spec.update(plane_pitch=NWNO + 3 if full else NWNO, flx=0)
    return resident.thermal_SH, kw, "picaso_get_thermal_SH_dev", spec


def case_reflected_3d(ck, weights):
    pl = _planes(REFLECTED_PLANES, skip=("tau", "tau_og", "gcos2"))
    rs, f0, x, alb = Dev(NWNO), Dev(NWNO), Dev(1), Dev(NWNO)
    kw = dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, numg=NG, numt=NT, planes=pl, surf_reflect=rs, ubar0=U0, ubar1=U1,
              cos_theta=0.7, F0PI=f0, **TTHG, xint_at_top=x)
    opts = dict(gweight=GW, tweight=TW, albedo=alb) if weights else dict(gweight=None, tweight=None, albedo=None)
    kw.update(opts if weights else {})
    spec = dict(kw, **{k + ("" if ck else "_3d"): pl.get(k) for k in REFLECTED_PLANES}, **opts)
    del spec["planes"]
    if ck:
        kw = dict(list(kw.items())[:3] + [("ngauss", NGAUSS)] + list(kw.items())[3:])
        i = list(kw).index("xint_at_top")
        kw = dict(list(kw.items())[:i] + [("gauss_wts", WTS)] + list(kw.items())[i:])
        spec.update(ngauss=NGAUSS, gauss_wts=WTS)
        return resident.reflected_3d_ck, kw, "picaso_get_reflected_3d_ck_dev", spec
    return resident.reflected_3d, kw, "picaso_get_reflected_3d_dev", spec


def case_thermal_3d(ck, weights):
    wno, dtau, w0, cosb, rs, x = Dev(NWNO), Dev(1), Dev(1), Dev(1), Dev(NWNO), Dev(1)
    opts = dict(gweight=GW, tweight=TW, flux_disk=Dev(NWNO)) if weights else dict(gweight=None, tweight=None, flux_disk=None)
    if ck:
        kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, ngauss=NGAUSS, numg=NG, numt=NT, tlevel_3d=TL3, dtau=dtau, w0=w0,
                  cosb=cosb, plevel_3d=PL3, ubar1=U1, surf_reflect=rs, hard_surface=1, gauss_wts=WTS, int_at_top=x)
    else:
        kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, numg=NG, numt=NT, tlevel_3d=TL3, dtau_3d=dtau, w0_3d=w0,
                  cosb_3d=cosb, plevel_3d=PL3, ubar1=U1, surf_reflect=rs, hard_surface=1, int_at_top=x)
    spec = dict(kw, **opts)
    kw.update(opts if weights else {})
    return ((resident.thermal_3d_ck, kw, "picaso_get_thermal_3d_ck_dev", spec) if ck
            else (resident.thermal_3d, kw, "picaso_get_thermal_3d_dev", spec))


def case_thermal_3d_batch(fuse, cloud):
    wno, rs = Dev(NWNO), Dev(NWNO)
    dtau, w0, cosb, fx, disk = (_devs(NSPEC, 1) for _ in range(5))
    kw = dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, numg=NG, numt=NT, tlevel_3d=TL3S, dtau_3d=dtau, w0_3d=w0,
              cosb_3d=cosb if cloud else None, plevel_3d=PL3S, ubar1=U1S if cloud else U1, surf_reflect=rs, hard_surface=1,
              int_at_top=fx)
    kw.update(dict(gweight=GW, tweight=TW, flux_disk=disk) if fuse else dict(gweight=GW, tweight=TW))
    spec = dict(kw, nspec=NSPEC, ubar1=U1S if cloud else np.broadcast_to(U1, (NSPEC, NG, NT)), surf_reflect=[rs] * NSPEC,
                gweight=GW if fuse else None, tweight=TW if fuse else None, flux_disk=disk if fuse else None)
    return resident.thermal_3d_batch, kw, "picaso_get_thermal_3d_batch_dev", spec


def case_small(which):
    x, y, out = Dev(5, 4), Dev(5, 4), Dev(5, 4)
    if which == "axpby":
        return (resident.axpby, dict(ctx=CTX, a=0.25, x=x, b=0.75, y=y, out=out), "picaso_axpby_dev",
                dict(ctx=CTX, n=20, a=0.25, x=x, b=0.75, y=y, out=out))
    if which == "trapz":
        kw = dict(ctx=CTX, n=NWNO, d=x, y=y, out=out)
        return resident.trapz, kw, "picaso_trapz_dev", dict(kw, mult=None, reverse=0)
    if which == "trapz-reverse":
        m = Dev(1)
        kw = dict(ctx=CTX, n=NWNO, d=x, y=y, out=out, mult=m, reverse=True)
        return resident.trapz, kw, "picaso_trapz_dev", dict(kw, reverse=1)
    if which == "compress_disco":
        f0 = Dev(NWNO)
        kw = dict(ctx=CTX, nwno=NWNO, cos_theta=0.7, xint_at_top=x, gweight=GW, tweight=TW, F0PI=f0, albedo=out)
        return resident.compress_disco, kw, "picaso_compress_disco_dev", dict(kw, ng=NG, nt=NT)
    if which == "compress_thermal":
        kw = dict(ctx=CTX, ninner=NLEVEL * NWNO, flux_at_top=x, gweight=GW, tweight=TW, flux=out)
        return resident.compress_thermal, kw, "picaso_compress_thermal_dev", dict(kw, ng=NG, nt=NT)
    lay = NLEVEL - 1
    kw = dict(ctx=CTX, z=TL + 1, dz=TL + 2, nlevel=NLEVEL, nwno=NWNO, ngauss=NGAUSS, rstar=6.9e10, mmw=TL[:lay] + 3, k_b=1.38e-16,
              amu=1.66e-24, player=PL[:lay], tlayer=TL[:lay] + 4, colden=TL[:lay] + 5, dtau=x, gauss_wts=WTS, rprs2=out)
    return resident.transit_1d_ck, kw, "picaso_get_transit_1d_ck_dev", dict(kw)


CASES = {
    "reflected_1d": lambda: case_reflected_1d(),
    "reflected_1d-weights-pitch": lambda: case_reflected_1d(weights=True),
    "thermal_1d": lambda: case_thermal_1d(),
    "thermal_1d-full": lambda: case_thermal_1d(full=True),
    "reflected_1d_batch-one-geometry-fused": lambda: case_reflected_1d_batch(False, True),
    "reflected_1d_batch-geometries-not-fused": lambda: case_reflected_1d_batch(True, False),
    "thermal_1d_batch-one-geometry-fused": lambda: case_thermal_1d_batch(False, True),
    "thermal_1d_batch-geometries-not-fused": lambda: case_thermal_1d_batch(True, False),
    "reflected_1d_ck": lambda: case_reflected_1d_ck(False),
    "reflected_1d_ck-lvl": lambda: case_reflected_1d_ck(True),
    "thermal_1d_ck": lambda: case_thermal_1d_ck(False),
    "thermal_1d_ck-lvl": lambda: case_thermal_1d_ck(True),
    "thermal_1d_ck_tbatch": lambda: case_tbatch(False),
    "thermal_nets_tbatch": lambda: case_tbatch(True),
    "reflected_SH": lambda: case_reflected_SH(),
    "reflected_SH-full": lambda: case_reflected_SH(full=True),
    "reflected_SH_batch-one-geometry-fused": lambda: case_reflected_SH_batch(False, True),
    "reflected_SH_batch-geometries-not-fused": lambda: case_reflected_SH_batch(True, False),
    "reflected_SH_ck": lambda: case_reflected_SH_ck(False),
    "reflected_SH_ck-full": lambda: case_reflected_SH_ck(True),
    "thermal_SH_ck": lambda: case_thermal_SH(True, False),
    "thermal_SH_ck-full": lambda: case_thermal_SH(True, True),
    "reflected_3d": lambda: case_reflected_3d(False, False),
    "reflected_3d-weights": lambda: case_reflected_3d(False, True),
    "reflected_3d_ck": lambda: case_reflected_3d(True, False),
    "reflected_3d_ck-weights": lambda: case_reflected_3d(True, True),
    "thermal_3d": lambda: case_thermal_3d(False, False),
    "thermal_3d-weights": lambda: case_thermal_3d(False, True),
    "thermal_3d_ck": lambda: case_thermal_3d(True, False),
    "thermal_3d_ck-weights": lambda: case_thermal_3d(True, True),
    "reflected_3d_batch-fused": lambda: case_reflected_3d_batch(True),
    "reflected_3d_batch-not-fused": lambda: case_reflected_3d_batch(False),
    "thermal_3d_batch-fused-cloud": lambda: case_thermal_3d_batch(True, True),
    "thermal_3d_batch-not-fused-clear": lambda: case_thermal_3d_batch(False, False),
    "axpby": lambda: case_small("axpby"),
    "trapz": lambda: case_small("trapz"),
    "trapz-reverse": lambda: case_small("trapz-reverse"),
    "compress_disco": lambda: case_small("compress_disco"),
    "compress_thermal": lambda: case_small("compress_thermal"),
    "transit_1d_ck": lambda: case_small("transit"),
    # the keyword surface the spectrum path needs: level fluxes, the SH layer fluxes, the monochromatic thermal SH solver
    "reflected_1d-lvl_fluxes": lambda: case_reflected_1d(weights=True, lvl=True),
    "reflected_SH-flux": lambda: case_reflected_SH(full=True, flux=True),
    "thermal_SH": lambda: case_thermal_SH(False, False),
    "thermal_SH-full": lambda: case_thermal_SH(False, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_wrapper_pins_every_argument_by_header_name(rec, name):
    fn, kw, func, spec = CASES[name]()
    _call(fn, kw)
    assert len(rec.calls) == 1
    _verify(rec.calls[0], func, spec)


def _slabs(arrs, step=None):
    """Facet slabs of facet-major arrays, spectrum by spectrum."""
    return [a.addr + f * (a.nbytes // NFAC if step is None else step) for a in arrs for f in range(NFAC)]


@pytest.mark.parametrize("fuse", [True, False])
def test_reflected_3d_fm_batch(rec, fuse):
    """Every facet of every spectrum is a spectrum of one facet in the batched launch; the disk sums follow."""
    present = [k for k in REFLECTED_PLANES if k not in ("tau", "tau_og", "gcos2")]
    pls = [{k: Dev(NFAC, NLEVEL, NWNO) for k in present} for _ in range(NSPEC)]
    rs, f0s, xs, albs = Dev(NWNO), _devs(NSPEC, NWNO), _devs(NSPEC, NG, NT, NWNO), _devs(NSPEC, NWNO)
    _call(resident.reflected_3d_fm_batch,
          dict(ctx=CTX, nlevel=NLEVEL, nwno=NWNO, numg=NG, numt=NT, planes=pls, surf_reflect=rs, ubar0=U0S, ubar1=U1S,
               cos_theta=CTS, F0PI=f0s, **TTHG, xint_at_top=xs, gweight=GW if fuse else None, tweight=TW, albedo=albs))
    spec = dict(ctx=CTX, nspec=NSPEC * NFAC, nlevel=NLEVEL, nwno=NWNO, numg=1, numt=1,
                **{k + "_3d": (_slabs([pl[k] for pl in pls]) if k in present else None) for k in REFLECTED_PLANES},
                surf_reflect=[rs] * (NSPEC * NFAC), ubar0=U0S, ubar1=U1S, cos_theta=np.repeat(CTS, NFAC),
                F0PI=[f for f in f0s for _ in range(NFAC)], **TTHG, xint_at_top=_slabs(xs, 8 * NWNO), gweight=None,
                tweight=None, albedo=None)
    _verify(rec.calls[0], "picaso_get_reflected_3d_batch_dev", spec)
    assert len(rec.calls) == 1 + (NSPEC if fuse else 0)
    for s, call in enumerate(rec.calls[1:]):
        _verify(call, "picaso_compress_disco_dev",
                dict(ctx=CTX, nwno=NWNO, cos_theta=CTS[s], xint_at_top=xs[s], gweight=GW, ng=NG, tweight=TW, nt=NT,
                     F0PI=f0s[s], albedo=albs[s]))


@pytest.mark.parametrize("fuse,cloud", [(True, True), (False, False)])
def test_thermal_3d_fm_batch(rec, fuse, cloud):
    wno, rs = Dev(NWNO), Dev(NWNO)
    dtau, w0, cosb = (_devs(NSPEC, NFAC, NLEVEL - 1, NWNO) for _ in range(3))
    fx, disk = _devs(NSPEC, NG, NT, NWNO), _devs(NSPEC, NWNO)
    _call(resident.thermal_3d_fm_batch,
          dict(ctx=CTX, nlevel=NLEVEL, wno=wno, nwno=NWNO, numg=NG, numt=NT, tlevel_3d=TL3S, dtau=dtau, w0=w0,
               cosb=cosb if cloud else None, plevel_3d=PL3S, ubar1=U1S, surf_reflect=rs, hard_surface=1, int_at_top=fx,
               gweight=GW, tweight=TW, flux_disk=disk if fuse else None))

    def by_facet(a):               # (nspec, nlevel, numg, numt) -> one (nlevel,) column per facet of every spectrum
        return np.ascontiguousarray(np.transpose(a.reshape(NSPEC, NLEVEL, NFAC), (0, 2, 1)))
    spec = dict(ctx=CTX, nspec=NSPEC * NFAC, nlevel=NLEVEL, wno=wno, nwno=NWNO, numg=1, numt=1, tlevel_3d=by_facet(TL3S),
                dtau_3d=_slabs(dtau), w0_3d=_slabs(w0), cosb_3d=_slabs(cosb) if cloud else None, plevel_3d=by_facet(PL3S),
                ubar1=U1S, surf_reflect=[rs] * (NSPEC * NFAC), hard_surface=1, int_at_top=_slabs(fx, 8 * NWNO),
                gweight=None, tweight=None, flux_disk=None)
    _verify(rec.calls[0], "picaso_get_thermal_3d_batch_dev", spec)
    assert len(rec.calls) == 1 + (NSPEC if fuse else 0)
    for s, call in enumerate(rec.calls[1:]):
        _verify(call, "picaso_compress_thermal_dev",
                dict(ctx=CTX, ninner=NWNO, flux_at_top=fx[s], gweight=GW, ng=NG, tweight=TW, nt=NT, flux=disk[s]))


def test_header_names_every_parameter():
    protos = _lib.declared_prototypes()
    assert set(PARAMS) == set(protos)
    for func, names in PARAMS.items():
        assert len(names) == len(protos[func][1])
        assert all(n.isidentifier() for n in names), func
        assert len(set(names)) == len(names), func
