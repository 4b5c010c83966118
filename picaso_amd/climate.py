"""Radiative-transfer call of the climate solver on the GPU: ``get_fluxes``.

Drop-in for the reference's ``climate.get_fluxes`` (picaso/climate.py:1687-1952), the function its
T(P) iteration evaluates on every Newton step: Toon reflected light at the two-stream angle
``ubar = 0.5`` and Toon thermal emission with bin-integrated Planck functions (``calc_type=1``),
both returning level and layer-midpoint fluxes for every correlated-k Gauss point, then the
Gauss-weight, patchy-cloud, disk and wavenumber sums.  Same positional arguments (the reference's
namedtuples or anything with the same attribute names) and the same eight arrays back.

Here the ``ngauss`` loop is one launch over ``nwno*ngauss`` columns per solver
(``picaso_get_reflected_1d_ck_dev`` / ``picaso_get_thermal_1d_ck_dev``, level-flux kernels of
``toon_lvl.hip``), the cloudy/clear blend and the disk quadrature run on the device, and only the
``(nlevel, nwno)`` results come back for the final wavenumber sums.
"""
from collections import namedtuple

import os

import numpy as np

from . import _lib, resident
from ._lib import f64
from .deq_chem import get_quench_levels
from .device import DeviceArray, PinnedArray

# the reference's containers (climate.py:1962-1966)
Atmosphere_Tuple = namedtuple("Atmosphere_Tuple", ["dtdp", "mmw_layer", "nlevel", "t_level", "p_level", "condensables",
                                                   "condensable_abundances", "condensable_weights", "scale_height"])
OpacityWEd_Tuple = namedtuple("OpacityWEd_Tuple", ["DTAU", "TAU", "W0", "COSB", "ftau_cld", "ftau_ray", "GCOS2",
                                                   "W0_no_raman", "f_deltaM"])
OpacityNoEd_Tuple = namedtuple("OpacityNoEd_Tuple", ["DTAU", "TAU", "W0", "COSB"])
ScatteringPhase_Tuple = namedtuple("ScatteringPhase_Tuple", ["surf_reflect", "single_phase", "multi_phase", "frac_a",
                                                             "frac_b", "frac_c", "constant_back", "constant_forward"])
Disco_Tuple = namedtuple("Disco_Tuple", ["ng", "nt", "gweight", "tweight", "ubar0", "ubar1", "cos_theta"])
# tmin / tmax: the temperature range of the opacity grid, which t_start keeps its trial profiles inside
Opagrid_Tuple = namedtuple("Opagrid_Tuple", ["nwno", "delta_wno", "wno", "ngauss", "gauss_wts", "tmin", "tmax"],
                           defaults=(-np.inf, np.inf))


@_lib.serialized
def calculate_atm(bundle, opacityclass, only_atmosphere=False):
    """Atmosphere set-up and opacities of one climate iteration (reference ``climate.calculate_atm``,
    climate.py:1969-2135): returns ``OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Atmosphere,
    (OpacityWEd_hole, OpacityNoEd_hole)`` with the reference's namedtuples.  The opacity planes are
    HBM-resident ``DeviceArray`` objects ``(nlayer|nlevel, nwno, ngauss)`` -- ``get_fluxes`` takes them as
    they are (``.to_host()`` gives the reference's numpy arrays)."""
    from . import justdoit, optics
    inputs = bundle.inputs
    opa = opacityclass
    common = inputs["approx"]["rt_params"]["common"]
    toon = inputs["approx"]["rt_params"]["toon"]
    frac_a, frac_b, frac_c = common["TTHG_params"]["fraction"]
    geom = inputs["disco"]
    do_holes = bool(inputs["clouds"].get("do_holes", False))
    atm = justdoit._setup_atmosphere(inputs, opa, opa.wno)
    atm.surf_reflect = 0                                   # climate.py:2052
    atm.get_dtdp()
    prof = inputs["atmosphere"]["profile"]
    ours = [m for m in ("H2O", "CH4", "NH3", "Fe") if m in prof.keys()]                  # :2090-2093
    Atmosphere = Atmosphere_Tuple(atm.layer["dtdp"], atm.layer["mmw"], atm.c.nlevel,
                                  np.ascontiguousarray(atm.level["temperature"]).copy(),
                                  np.ascontiguousarray(atm.level["pressure_bar"]).copy(), ours,
                                  np.array([np.asarray(prof[m], dtype=float) for m in ours]),
                                  [atm.weights[m] for m in ours], atm.level["scale_height"])
    if only_atmosphere:
        return Atmosphere
    opa.get_opacities(atm)
    kw = dict(ngauss=opa.ngauss, stream=common["stream"], delta_eddington=common["delta_eddington"],
              test_mode=inputs["test_mode"], raman=common["raman"])

    def tuples(pl):
        return (OpacityWEd_Tuple(pl["dtau"], pl["tau"], pl["w0"], pl["cosb"], pl["ftau_cld"], pl["ftau_ray"],
                                 pl["gcos2"], pl["w0_no_raman"], pl["f_deltaM"]),
                OpacityNoEd_Tuple(pl["dtau_og"], pl["tau_og"], pl["w0_og"], pl["cosb_og"]))
    holes = (None, None)
    if do_holes:                                           # :2104-2112
        holes = tuples(optics.compute_opacity_resident(atm, opa, fthin_cld=inputs["clouds"]["fthin_cld"],
                                                       do_holes=True, **kw))
    wed, noed = tuples(optics.compute_opacity_resident(atm, opa, **kw))
    sp = ScatteringPhase_Tuple(atm.surf_reflect, toon["single_phase"], toon["multi_phase"], frac_a, frac_b, frac_c,
                               common["TTHG_params"]["constant_back"], common["TTHG_params"]["constant_forward"])
    dis = Disco_Tuple(geom["num_gangle"], geom["num_tangle"], geom["gweight"], geom["tweight"], geom["ubar0"],
                      geom["ubar1"], geom["cos_theta"])
    return wed, noed, sp, dis, Atmosphere, holes


def _planes(wed, noed, ctx, thermal_only=False):
    """Upload the (rows, nwno, ngauss) arrays of one opacity set (DeviceArrays pass through)."""
    def up(x):
        return x if isinstance(x, DeviceArray) else DeviceArray.from_host(f64(x), ctx)
    pl = {"dtau_og": up(noed.DTAU), "w0_no_raman": up(wed.W0_no_raman), "cosb_og": up(noed.COSB)}
    if not thermal_only:
        pl.update(dtau=up(wed.DTAU), tau=up(wed.TAU), w0=up(wed.W0), cosb=up(wed.COSB), gcos2=up(wed.GCOS2),
                  ftau_cld=up(wed.ftau_cld), ftau_ray=up(wed.ftau_ray), tau_og=up(noed.TAU), w0_og=up(noed.W0))
    return pl


_VEC_CACHE = {}          # (pid, context, bytes) -> DeviceArray; entries of a context go when it is destroyed
_lib.on_context_destroy(lambda value: [_VEC_CACHE.pop(k) for k in [k for k in _VEC_CACHE if k[1] == value]])


def _resident_small(values, ctx):
    """A per-wavelength host vector as a resident one, kept by content: the T(P) iteration calls get_fluxes thousands of
    times with the same wavenumbers, bin widths, stellar flux and surface reflectivity (four 5 KB uploads per call,
    0.06 ms each)."""
    a = np.ascontiguousarray(values, dtype=np.float64)
    key = (os.getpid(), getattr(ctx, "value", ctx), a.tobytes())
    hit = _VEC_CACHE.get(key)
    if hit is None:
        while len(_VEC_CACHE) >= 64:               # oldest first
            del _VEC_CACHE[next(iter(_VEC_CACHE))]
        hit = _VEC_CACHE[key] = DeviceArray.from_host(a, ctx)
    return hit


@_lib.serialized
def get_fluxes(Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid, F0PI, reflected, thermal,
               do_holes=False, fhole=0.0, hole_OpacityWEd=None, hole_OpacityNoEd=None, ctx=None,
               copy_outputs=False):
    """Visible and IR net (layer and level), upward and downward fluxes (reference
    ``climate.get_fluxes``, climate.py:1687-1952).  Returns ``flux_net_v_layer, flux_net_v, flux_plus_v,
    flux_minus_v, flux_net_ir_layer, flux_net_ir, flux_plus_ir, flux_minus_ir``.

    ``flux_plus_v`` / ``flux_minus_v`` are ``(ng, nt, nlevel, nwno)`` as in the reference, where every
    disk angle holds the same two-stream result (climate.py:1803-1805, :1868-1869); here they are
    read-only broadcast views of that one ``(nlevel, nwno)`` array (the climate solver reads
    ``[0, 0, :, :]``, climate.py:946-947) unless ``copy_outputs=True`` asks for writable copies."""
    ctx = ctx if ctx is not None else _lib.context()
    pressure, temperature, nlevel = Atmosphere.p_level, Atmosphere.t_level, int(Atmosphere.nlevel)
    sp = ScatteringPhase
    ng, nt = int(Disco.ng), int(Disco.nt)
    nwno, ngauss = int(Opagrid.nwno), int(Opagrid.ngauss)
    dwni, wno, gauss_wts = f64(Opagrid.delta_wno), f64(Opagrid.wno), f64(Opagrid.gauss_wts)
    if do_holes and (hole_OpacityWEd is None or hole_OpacityNoEd is None):
        raise Exception("get_fluxes: do_holes=True needs hole_OpacityWEd and hole_OpacityNoEd")

    flux_net_v = np.zeros((ng, nt, nlevel))
    flux_net_v_layer = np.zeros((ng, nt, nlevel))
    flux_plus_v = flux_minus_v = None
    flux_net_ir = np.zeros(nlevel)
    flux_net_ir_layer = np.zeros(nlevel)
    flux_plus_ir = np.zeros((nlevel, nwno))
    flux_minus_ir = np.zeros((nlevel, nwno))

    rs = _resident_small(np.zeros(nwno) + f64(sp.surf_reflect), ctx)
    if thermal:                                           # uploaded (first use) before the second stream is ordered behind this one
        d_wno, d_dw = _resident_small(wno, ctx), _resident_small(dwni, ctx)
    sets = [_planes(OpacityWEd, OpacityNoEd, ctx, thermal_only=not reflected)]
    if do_holes:
        sets.append(_planes(hole_OpacityWEd, hole_OpacityNoEd, ctx, thermal_only=not reflected))

    def blend(results, c):                                # (1-fhole)*cloudy + fhole*clear, climate.py:1838-1842
        if len(results) == 1:
            return results[0]
        for a, b in zip(*results):
            resident.axpby(c, 1.0 - fhole, a, fhole, b, a)
        return results[0]

    # both legs are small launches (661 bins x 8 Gauss points = 83 waves on a 1 024-SIMD chip, one 90-layer chain each):
    # the thermal leg goes to the process's second stream, behind the uploads above, and runs next to the reflected one
    tctx = ctx
    if reflected and thermal and os.environ.get("PICASO_AMD_OVERLAP_LEGS", "1") != "0":
        tctx = _lib.aux_context(_lib.device_of(ctx))
        _lib.ctx_wait(tctx, ctx)

    if reflected:                                         # climate.py:1796-1874
        d_f0 = _resident_small(np.zeros(nwno) + f64(F0PI), ctx)
        half = np.full((1, 1), 0.5)                       # ubar0_clima = ubar1_clima = 0.5, one angle
        xdummy = DeviceArray((1, 1, nwno), ctx)
        res = []
        for pl in sets:
            stack = DeviceArray((4, 1, 1, nlevel, nwno), ctx)       # one buffer, one copy back
            lv = [stack.row_block(k) for k in range(4)]
            resident.reflected_1d_ck(ctx, nlevel, nwno, ngauss, 1, 1, pl, rs, half, half, float(Disco.cos_theta),
                                     d_f0, int(sp.single_phase), int(sp.multi_phase), float(sp.frac_a),
                                     float(sp.frac_b), float(sp.frac_c), float(sp.constant_back),
                                     float(sp.constant_forward), gauss_wts, xdummy, get_toa_intensity=0,
                                     lvl_fluxes=lv)
            res.append(lv)
        refl_stack = blend(res, ctx)[0]._owner            # read back after the thermal leg is enqueued
        refl_pin = refl_stack.to_host_async(PinnedArray(refl_stack.shape, ctx))     # the copy: behind the leg's last kernel

    if thermal:                                           # climate.py:1879-1941
        xdummy = DeviceArray((ng, nt, nwno), tctx)
        res = []
        for pl in sets:
            lv = [DeviceArray((ng, nt, nlevel, nwno), tctx) for _ in range(4)]
            resident.thermal_1d_ck(tctx, nlevel, d_wno, nwno, ngauss, ng, nt, temperature, pl["dtau_og"],
                                   pl["w0_no_raman"], pl["cosb_og"], pressure, Disco.ubar1, rs, 0, gauss_wts,
                                   xdummy, dwno=d_dw, calc_type=1, lvl_fluxes=lv)
            res.append(lv)
        disk = DeviceArray((4, nlevel, nwno), tctx)
        for k, x in enumerate(blend(res, tctx)):          # compress_thermal over the disk angles (:1925-1928)
            resident.compress_thermal(tctx, nlevel * nwno, x, Disco.gweight, Disco.tweight, disk.row_block(k))
        therm_pin = disk.to_host_async(PinnedArray(disk.shape, tctx))

    # both legs are on the stream before the first copy back (each copy is a synchronisation)
    if reflected:
        fm, fp, fmm, fpm = refl_pin.wait().copy()         # Gauss-weighted (1,1,nlevel,nwno) each
        refl_pin.free()
        flux_net_v_layer += np.sum(fpm, axis=3) - np.sum(fmm, axis=3)
        flux_net_v += np.sum(fp, axis=3) - np.sum(fm, axis=3)
        # the single two-stream angle stands for every disk angle (climate.py:1803-1805, :1868-1869)
        flux_plus_v = np.broadcast_to(fp, (ng, nt, nlevel, nwno))
        flux_minus_v = np.broadcast_to(fm, (ng, nt, nlevel, nwno))
        if copy_outputs:
            flux_plus_v, flux_minus_v = flux_plus_v.copy(), flux_minus_v.copy()
    if thermal:
        fm, fp, fmm, fpm = therm_pin.wait()
        flux_net_ir_layer = ((fpm - fmm) * dwni).sum(axis=1)                  # (:1931-1936)
        flux_net_ir = ((fp - fm) * dwni).sum(axis=1)
        flux_plus_ir = fp * dwni
        flux_minus_ir = fm * dwni
        therm_pin.free()

    if flux_plus_v is None:
        flux_plus_v, flux_minus_v = np.zeros((ng, nt, nlevel, nwno)), np.zeros((ng, nt, nlevel, nwno))
    return (flux_net_v_layer, flux_net_v, flux_plus_v, flux_minus_v, flux_net_ir_layer, flux_net_ir,
            flux_plus_ir, flux_minus_ir)


@_lib.serialized
def get_fluxes_tbatch(temperatures, Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid, ctx=None,
                      chunk=32, nets_only=False):
    """The IR half of ``get_fluxes`` (``reflected=False, thermal=True``) for every level-temperature profile in
    ``temperatures`` ``(nitem, nlevel)`` over ONE set of opacities: ``flux_net_ir_layer, flux_net_ir`` ``(nitem, nlevel)``
    and ``flux_plus_ir, flux_minus_ir`` ``(nitem, nlevel, nwno)``.

    What it is for: the Jacobian of the reference's T(P) iteration perturbs one level temperature at a time, rebuilds
    the profile and calls ``get_fluxes`` with the SAME opacities (climate.py:1105-1180: ~nlevel calls per Newton step,
    each a Planck evaluation + two-stream solve + source-function sweeps).  Here the profiles are extra columns of one
    launch sequence (``picaso_get_thermal_1d_ck_tbatch_dev``: a column reads the shared planes and its own profile's
    level temperatures); ``chunk`` profiles at a time bound the scratch (91 levels x 661 bins x 8 Gauss points x 5 angles:
    77 MB per profile).  Row ``k`` of every result equals ``get_fluxes(Atmosphere._replace(t_level=temperatures[k]), ...)``
    bit for bit (same kernels per column, same numpy sums).  Patchy clouds (``do_holes``) blend the cloudy and the clear
    column sets before the disk sum: call ``get_fluxes`` per profile for those.

    ``nets_only=True`` (what the Jacobian reads, climate.py:1182-1185): only ``flux_net_ir_layer, flux_net_ir`` come back,
    summed over wavenumber ON THE DEVICE (``picaso_flux_net_sums_dev``: a fixed tree per row instead of numpy's order, so
    they agree with ``get_fluxes`` to ~1e-15 relative instead of bit for bit) -- 2 x nlevel doubles per profile cross
    PCIe instead of 4 x nlevel x nwno."""
    ctx = ctx if ctx is not None else _lib.context()
    temps = f64(temperatures)
    nlevel = int(Atmosphere.nlevel)
    if temps.ndim != 2 or temps.shape[1] != nlevel:
        raise Exception("get_fluxes_tbatch: temperatures must be (nitem, nlevel=%d)" % nlevel)
    nitem = temps.shape[0]
    sp = ScatteringPhase
    ng, nt = int(Disco.ng), int(Disco.nt)
    nwno, ngauss = int(Opagrid.nwno), int(Opagrid.ngauss)
    dwni, wno, gauss_wts = f64(Opagrid.delta_wno), f64(Opagrid.wno), f64(Opagrid.gauss_wts)
    rs = _resident_small(np.zeros(nwno) + f64(sp.surf_reflect), ctx)
    pl = _planes(OpacityWEd, OpacityNoEd, ctx, thermal_only=True)
    d_wno, d_dw = _resident_small(wno, ctx), _resident_small(dwni, ctx)
    net_layer, net = np.empty((nitem, nlevel)), np.empty((nitem, nlevel))
    plus = minus = None
    if not nets_only:
        plus, minus = np.empty((nitem, nlevel, nwno)), np.empty((nitem, nlevel, nwno))
    for c0 in range(0, nitem, max(1, int(chunk))):
        tl = temps[c0:c0 + max(1, int(chunk))]
        m = tl.shape[0]
        disk4 = DeviceArray((4, nlevel, m * nwno), ctx)
        resident.thermal_1d_ck_tbatch(ctx, nlevel, d_wno, nwno, ngauss, ng, nt, tl, pl["dtau_og"], pl["w0_no_raman"],
                                      pl["cosb_og"], Atmosphere.p_level, Disco.ubar1, rs, 0, gauss_wts, Disco.gweight,
                                      Disco.tweight, disk4, dwno=d_dw, calc_type=1)
        if nets_only:
            d_nl, d_n = DeviceArray((m, nlevel), ctx), DeviceArray((m, nlevel), ctx)
            _lib.check(_lib.load().picaso_flux_net_sums_dev(ctx, nlevel, m, nwno, disk4.addr, d_dw.addr, d_nl.addr, d_n.addr),
                       ctx)
            net_layer[c0:c0 + m], net[c0:c0 + m] = d_nl.to_host(), d_n.to_host()
            continue
        fm, fp, fmm, fpm = disk4.to_host().reshape(4, nlevel, m, nwno)
        for k in range(m):                                     # get_fluxes' own expressions (climate.py:1931-1936)
            net_layer[c0 + k] = ((fpm[:, k] - fmm[:, k]) * dwni).sum(axis=1)
            net[c0 + k] = ((fp[:, k] - fm[:, k]) * dwni).sum(axis=1)
            plus[c0 + k] = fp[:, k] * dwni
            minus[c0 + k] = fm[:, k] * dwni
    if nets_only:
        return net_layer, net
    return net_layer, net, plus, minus


# ---------------------------------------------------------------------------------------------------------------------
# The T(P) iteration (reference climate.t_start, climate.py:805-1552) and its helpers.  Host code: the device work of a
# Newton step is the flux calls, everything else is O(nlevel^2) arithmetic.
# ---------------------------------------------------------------------------------------------------------------------
AdiabatBundle_Tuple = namedtuple("AdiabatBundle_Tuple", ["t_table", "p_table", "grad", "cp"])
convergence_criteriaT = namedtuple("Conv", ["it_max", "itmx", "conv", "convt", "x_max_mult"])     # climate.py:21
MAX_LEVELS = 128         # the limit the contribution kernels state; mat_sol has no NMAX = 100 / int8 index limit


def load_adiabat(path=None):
    """The H/He adiabat table of the reference (justdoit.py:1726-1735): log10 T (K), log10 P (bar), the adiabatic
    gradient d ln T / d ln P and log10 cp (erg/g/K) -> ``AdiabatBundle_Tuple``.  ``path=None`` reads
    ``$picaso_refdata/climate_INPUTS/specific_heat_p_adiabat_grad.json``."""
    import json
    if path is None:
        ref = os.environ.get("picaso_refdata")
        if ref is None:
            raise Exception("no file was given and the picaso_refdata environment variable is not set: the adiabat table "
                            "is looked up under $picaso_refdata/climate_INPUTS, as in the reference")
        path = os.path.join(ref, "climate_INPUTS", "specific_heat_p_adiabat_grad.json")
    with open(path) as fh:
        tab = json.load(fh)
    return AdiabatBundle_Tuple(np.array(tab["temperature"], dtype=float), np.array(tab["pressure"], dtype=float),
                               np.array(tab["adiabat_grad"], dtype=float), np.array(tab["specific_heat"], dtype=float))


def locate(array, value):
    """Index ``jl`` of the reference's bisection (climate.py:611-646): the last ``jl`` with ``array[jl] <= value``,
    0 at or below the first point, ``n - 1`` at or above the last.  ``value`` may be an array."""
    array = np.asarray(array)
    n = len(array)
    v = np.asarray(value, dtype=float)
    jl = np.clip(np.searchsorted(array, v, side="right") - 1, 0, n - 1)
    jl = np.where(np.isnan(v) | (v <= array[0]), 0, jl)          # a NaN fails every comparison of the bisection
    jl = np.where(v >= array[-1], n - 1, jl)
    return int(jl) if jl.ndim == 0 else jl.astype(np.intp)


def did_grad_cp(t, p, AdiabatBundle):
    """Adiabatic gradient and specific heat at temperature ``t`` (K) and pressure ``p`` (bar): bilinear in the table's
    log10 axes (reference climate.py:497-567).  As there, the first cell of either axis is not interpolated (the weight is
    0 below the second point) and points off the table take the edge.  ``t`` and ``p`` may be arrays of one shape."""
    t_table, p_table, grad, cp = (np.asarray(AdiabatBundle.t_table), np.asarray(AdiabatBundle.p_table),
                                  np.asarray(AdiabatBundle.grad), np.asarray(AdiabatBundle.cp))
    temp_log, pres_log = np.log10(np.asarray(t, dtype=float)), np.log10(np.asarray(p, dtype=float))

    def weights(table, x):
        last = len(table) - 1
        pos = np.asarray(locate(table, x))
        top = pos == last
        pos = np.where(top, last - 1, pos)
        with np.errstate(invalid="ignore"):
            fact = (-table[pos] + x) / (table[pos + 1] - table[pos])
        return pos, np.where(top, 1.0, np.where(pos == 0, 0.0, fact))
    pos_t, factkt = weights(t_table, temp_log)
    pos_p, factkp = weights(p_table, pres_log)

    def bilinear(z):
        return ((1.0 - factkt) * (1.0 - factkp) * z[pos_t, pos_p] + factkt * (1.0 - factkp) * z[pos_t + 1, pos_p]
                + factkt * factkp * z[pos_t + 1, pos_p + 1] + (1.0 - factkt) * factkp * z[pos_t, pos_p + 1])
    grad_x, cp_x = bilinear(grad), 10 ** bilinear(cp)
    if np.ndim(grad_x) == 0:
        return float(grad_x), float(cp_x)
    return grad_x, cp_x


def convec(temp, pressure, AdiabatBundle, Atmosphere, moist=False):
    """``grad_x, cp_x`` of every layer: ``did_grad_cp`` at the mean temperature and the geometric-mean pressure
    (reference climate.py:570-608)."""
    if moist:
        raise NotImplementedError("convec: the moist adiabat is not implemented")
    temp, pressure = f64(temp), f64(pressure)
    tbar = 0.5 * (temp[:-1] + temp[1:])
    pbar = np.sqrt(pressure[:-1] * pressure[1:])
    return did_grad_cp(tbar, pbar, AdiabatBundle)


def mat_sol(a, nlevel, nstrat, dflux):
    """Solve the leading ``nstrat x nstrat`` system of ``a`` for the right-hand side ``dflux[:nstrat]``, in place, and
    return ``a, dflux`` as the reference does (climate.py:650-802): LU decomposition with implicit row scaling, then
    back substitution.  The pivot of a column is the LAST row whose scaled magnitude reaches the maximum (``dum >= aamax``),
    and an exactly zero pivot becomes 1e-20.

    Rows at a time: the decomposition eliminates one column per step over all remaining rows, which gives every element
    the reference's subtractions in the reference's order; the substitutions run a running sum along each row."""
    n = int(nstrat)
    if not 0 < n <= int(nlevel) <= MAX_LEVELS:
        raise ValueError("mat_sol: needs 0 < nstrat <= nlevel <= %d, got nstrat=%d nlevel=%d" % (MAX_LEVELS, n, nlevel))
    m = a[:n, :n]                                                # a view: the caller's matrix holds the factors
    b = dflux
    aamax = np.abs(m).max(axis=1)
    if np.any(aamax == 0.0):
        raise ValueError("Array is singular, cannot be decomposed in n:" + str(n))
    vv = 1.0 / aamax
    indx = np.zeros(n, dtype=np.intp)
    imax = 0
    for j in range(n):
        dum = vv[j:] * np.abs(m[j:, j])
        hit = np.flatnonzero(dum >= np.fmax.reduce(dum, initial=0.0))        # a NaN row never compares >=
        if len(hit):
            imax = j + int(hit[-1])
        if imax != j:
            m[[j, imax]] = m[[imax, j]]
            vv[imax] = vv[j]
        indx[j] = imax
        if m[j, j] == 0:
            m[j, j] = 1e-20
        if j != n - 1:
            m[j + 1:, j] *= 1.0 / m[j, j]
            m[j + 1:, j + 1:] -= np.outer(m[j + 1:, j], m[j, j + 1:])
    for i in range(n):                                            # forward, unscrambling the permutation
        ll = indx[i]
        s = b[ll]
        b[ll] = b[i]
        b[i] = np.cumsum(np.concatenate(([s], -(m[i, :i] * b[:i]))))[-1]
    for i in range(n - 1, -1, -1):
        b[i] = np.cumsum(np.concatenate(([b[i]], -(m[i, i + 1:] * b[i + 1:n]))))[-1] / m[i, i]
    return a, b


def check_convergence(f_vec, n_total, tolf, check, f, dflux, tolmin, temp, temp_old, g, tolx):
    """The three exits of the line search (reference climate.py:1555-1631) -> ``flag_converge, check``: 2 when the
    largest residual is below ``tolf``, 2 on a step too small to continue (``check``: whether the gradient vanishes too),
    2 when the first ``n_total`` temperatures moved by less than ``tolx``; 1 otherwise (take another Newton step)."""
    n = int(n_total)
    def largest(x):                                               # of a running `if x > test`: from 0, NaNs passed over
        return np.fmax.reduce(x, initial=0.0)
    if largest(np.abs(f_vec[:n])) < tolf:
        return 2, False
    if check:
        den1 = max(f, 0.5 * n)
        return 2, bool(largest(np.abs(g[:n]) * dflux[:n] / den1) < tolmin)
    test = largest(np.abs(temp[:n] - temp_old[:n]) / temp_old[:n])
    if test < tolx:
        return 2, check
    return 1, check


def growup(nlv, nstr, ngrow):
    """Move the top of convective zone ``nlv`` up by ``ngrow`` levels (reference climate.py:1634-1652)."""
    nstr[3 * (nlv - 1) + 1] -= ngrow
    return nstr


def growdown(nlv, nstr, ngrow):
    """Move the bottom of convective zone ``nlv`` and the top of the radiative zone below it down by ``ngrow`` levels
    (reference climate.py:1655-1675)."""
    n = 3 * (nlv - 1) + 2
    nstr[n] += ngrow
    nstr[n + 1] += ngrow
    return nstr


@_lib.serialized
def get_nets_tbatch(temperatures, Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid, do_holes=False,
                    fhole=0.0, hole_OpacityWEd=None, hole_OpacityNoEd=None, ctx=None):
    """``flux_net_ir_layer, flux_net_ir`` ``(nitem, nlevel)`` of every level-temperature profile in ``temperatures``
    ``(nitem, nlevel)`` over one set of opacities: what ``t_start`` reads of a thermal ``get_fluxes`` call, for the
    perturbed profiles of a Jacobian in one batch and for a line-search trial with ``nitem = 1``.

    Patchy clouds (``do_holes``): the nets are linear in the fluxes, so the cloudy and the clear plane sets are run one
    after the other and their ``2 * nlevel`` numbers per profile are blended ``(1 - fhole) * cloudy + fhole * clear``
    here."""
    ctx = ctx if ctx is not None else _lib.context()
    if do_holes and (hole_OpacityWEd is None or hole_OpacityNoEd is None):
        raise Exception("get_nets_tbatch: do_holes=True needs hole_OpacityWEd and hole_OpacityNoEd")
    out = _nets_one_set(temperatures, Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid, ctx)
    if do_holes:
        clear = _nets_one_set(temperatures, Atmosphere, hole_OpacityWEd, hole_OpacityNoEd, ScatteringPhase, Disco, Opagrid,
                              ctx)
        out = tuple((1.0 - fhole) * a + fhole * b for a, b in zip(out, clear))
    return out


def _nets_one_set(temperatures, Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid, ctx):
    """One plane set of get_nets_tbatch: the fused kernel, or -- past the angle count it is compiled for -- the level
    planes of get_fluxes_tbatch summed on the device."""
    ng, nt = int(Disco.ng), int(Disco.nt)
    if ng * nt > resident.thermal_nets_max_angles():
        return get_fluxes_tbatch(temperatures, Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid,
                                 ctx=ctx, nets_only=True)
    temps = f64(temperatures)
    nlevel = int(Atmosphere.nlevel)
    if temps.ndim != 2 or temps.shape[1] != nlevel:
        raise Exception("get_nets_tbatch: temperatures must be (nitem, nlevel=%d)" % nlevel)
    nitem = temps.shape[0]
    nwno, ngauss = int(Opagrid.nwno), int(Opagrid.ngauss)
    rs = _resident_small(np.zeros(nwno) + f64(ScatteringPhase.surf_reflect), ctx)
    pl = _planes(OpacityWEd, OpacityNoEd, ctx, thermal_only=True)
    d_wno, d_dw = _resident_small(f64(Opagrid.wno), ctx), _resident_small(f64(Opagrid.delta_wno), ctx)
    both = DeviceArray((2, nitem, nlevel), ctx)
    resident.thermal_nets_tbatch(ctx, nlevel, d_wno, nwno, ngauss, ng, nt, temps, pl["dtau_og"], pl["w0_no_raman"],
                                 pl["cosb_og"], Atmosphere.p_level, Disco.ubar1, rs, 0, Opagrid.gauss_wts, Disco.gweight,
                                 Disco.tweight, d_dw, both.row_block(0), both.row_block(1))
    out = both.to_host()
    return out[0], out[1]


def _lapse(temp, pressure):
    return (np.log(temp[:-1]) - np.log(temp[1:])) / (np.log(pressure[:-1]) - np.log(pressure[1:]))


def t_start(nofczns, nstr, convergence_criteria, rfaci, rfacv, tidal, Atmosphere, OpacityWEd, OpacityNoEd,
            ScatteringPhase, Disco, Opagrid, AdiabatBundle, F0PI, save_profile, all_profiles, fhole=None,
            hole_OpacityWEd=None, hole_OpacityNoEd=None, verbose=1, do_holes=None, moist=False, egp_stepmax=False,
            ctx=None, _fluxes=None):
    """Newton-Raphson iteration on the level temperatures that zeroes the net flux in the radiative zones, with the
    opacities held fixed (reference ``climate.t_start``, climate.py:805-1552; same positional arguments).  Returns
    ``temp, dtdp, all_profiles, flux_net_ir, flux_net_v, flux_plus_ir[0, :]``; when ``it_max`` runs out the fourth value
    is ``flux_net_ir_layer``, as in the reference.

    ``nstr`` describes the zones: ``nstr[0]`` the top level (0), ``nstr[1]`` the last radiative level of the upper zone,
    ``nstr[2]`` the last layer of the convective zone below it, and ``nstr[3:6]`` the same for a second pair when
    ``nofczns = 2``.  The unknowns are the temperatures of the radiative levels; a convective zone continues the adiabat
    from the level above it (``did_grad_cp``).  The residuals are the net flux (``rfaci * IR + rfacv * visible + tidal``) at
    the top level and at the layer midpoints of the radiative zones.

    One step: every unknown is raised by ``max(1e-4 T, 3)`` K in turn and the profile rebuilt; the IR nets of ALL those
    profiles come from one batched call and give the finite-difference matrix ``A``; ``mat_sol`` solves ``A p = -f``; the
    step is capped (``egp_stepmax``: 0.005 of the temperature norm; otherwise a cap that is multiplied by that norm
    and by ``(it_max - its) / it_max`` every iteration); a backtracking line search on ``0.5 |f|^2`` follows, each trial one
    nets-only call, temperatures held inside ``(Opagrid.tmin, Opagrid.tmax)``, ended by ``check_convergence``.

    Calls: the first evaluation is ``get_fluxes(reflected=rfacv != 0, thermal=True)`` (the visible nets stay fixed); the
    Jacobian and the trials are ``get_nets_tbatch``; one thermal ``get_fluxes`` at the accepted profile gives the returned
    IR fluxes.  With ``do_holes`` each of them covers both plane sets.

    The caller's ``Atmosphere.t_level`` is NOT modified.  The reference writes its trial temperatures into that array
    and its callers use the returned one; use the returned ``temp`` here too.  ``moist=True`` (the moist adiabat) is not
    implemented.  ``nstr[0]`` must be 0, as every caller of the reference passes it.

    ``_fluxes=(single, batched)`` (tests): host callables in place of the two device calls, ``single`` with
    ``get_fluxes``' arguments and ``batched`` with ``get_nets_tbatch``'s (``None``: ``single`` per profile)."""
    if moist:
        raise NotImplementedError("t_start: the moist adiabat (moist=True) is not implemented")
    nstr = [int(x) for x in nstr]
    nofczns = int(nofczns)
    if nstr[0] != 0:
        raise ValueError("t_start: nstr[0] must be 0 (the top level)")
    pressure = f64(Atmosphere.p_level)
    temp = np.array(Atmosphere.t_level, dtype=np.float64)         # a copy: the working profile
    nlevel = len(temp)
    if nlevel > MAX_LEVELS:
        raise ValueError("t_start: at most %d levels" % MAX_LEVELS)
    tmin, tmax = Opagrid.tmin, Opagrid.tmax
    it_max = int(convergence_criteria.it_max)                     # the only field of the tuple this function reads
    tidal = f64(tidal)
    holes = {}
    if do_holes:
        holes = dict(do_holes=True, fhole=fhole, hole_OpacityWEd=hole_OpacityWEd, hole_OpacityNoEd=hole_OpacityNoEd)
    common = (OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid)
    if _fluxes is None:
        ctx = ctx if ctx is not None else _lib.context()

        def single(*a, **k):
            return get_fluxes(*a, ctx=ctx, **k)

        def batched(*a, **k):
            return get_nets_tbatch(*a, ctx=ctx, **k)
    else:
        single, batched = _fluxes
        if batched is None:
            def batched(temps, atm, *a, **k):
                rows = [single(atm._replace(t_level=t.copy()), *a, F0PI, False, True, **k) for t in temps]
                return np.array([r[4] for r in rows]), np.array([r[5] for r in rows])

    def nets(profiles):
        nl, n = batched(np.ascontiguousarray(profiles), Atmosphere, *common, **holes)
        return np.asarray(nl), np.asarray(n)

    # zones: the unknown levels n_top..n_strt, the adiabat levels n_strt+1..n_bot, and what a level index loses to
    # become an index of the solver's vectors
    zones, unknown, shift = [], [], 0
    for z in range(nofczns):
        n_top = nstr[3 * z] + (1 if z else 0)
        n_strt, n_bot = nstr[3 * z + 1], nstr[3 * z + 2] + 1
        zones.append((n_top, n_strt, n_bot, shift))
        unknown += list(range(n_top, n_strt + 1))
        shift = -1 + sum(zb - zs for _, zs, zb, _ in zones)
    unknown = np.array(unknown, dtype=np.intp)
    n_total = len(unknown)
    index = np.concatenate([np.arange(zt, zs + 1) - sh for zt, zs, _, sh in zones])     # 0..n_total-1 in a valid nstr
    if not np.array_equal(index, np.arange(n_total)) or (n_total and unknown.max() >= nlevel):
        raise ValueError("t_start: nstr does not describe contiguous zones: %r" % (nstr,))
    first = np.zeros(n_total, dtype=bool)
    first[0] = True
    dlogp = np.log(pressure[1:]) - np.log(pressure[:-1])           # log p[j] - log p[j-1], at j-1
    pmid = np.sqrt(pressure[:-1] * pressure[1:])

    def residual(net_ir, net_ir_layer):
        flux_net = rfaci * net_ir + rfacv * flux_net_v + tidal
        flux_net_midpt = rfaci * net_ir_layer + rfacv * flux_net_v_layer + tidal
        return np.where(first, flux_net[unknown], flux_net_midpt[unknown - 1]), flux_net

    def half_sum_sq(v):
        return 0.5 * np.cumsum(v ** 2)[-1]                         # a running sum, as the reference's loop

    def adiabat(t, zone, t_for_grad):
        """Continue the adiabat through one convective zone of `t`; the gradient is taken at `t_for_grad[j-1]`
        (None: at the level just computed)."""
        _, n_strt, n_bot, _ = zone
        if t_for_grad is not None and n_bot > n_strt:
            grads = did_grad_cp(t_for_grad[n_strt:n_bot], pmid[n_strt:n_bot], AdiabatBundle)[0]
        for j1 in range(n_strt + 1, n_bot + 1):
            gx = grads[j1 - 1 - n_strt] if t_for_grad is not None else did_grad_cp(t[j1 - 1], pmid[j1 - 1], AdiabatBundle)[0]
            t[j1] = np.exp(np.log(t[j1 - 1]) + gx * dlogp[j1 - 1])

    first_out = single(Atmosphere._replace(t_level=temp.copy()), *common, F0PI, rfacv != 0, True, **holes)
    flux_net_v_layer, flux_net_v = first_out[0][0, 0, :], first_out[1][0, 0, :]
    flux_net_ir_layer, flux_net_ir, flux_plus_ir = first_out[4], first_out[5], first_out[6]

    def finish(layer_in_fourth):
        out = single(Atmosphere._replace(t_level=temp.copy()), *common, F0PI, False, True, **holes)
        return temp, _lapse(temp, pressure), all_profiles, out[4] if layer_in_fourth else out[5], flux_net_v, out[6][0, :]

    eps, alf, tolmin, tolf, tolx = 1e-4, 1e-4, 1e-5, 5e-3, 5e-3
    step_max, alam2 = 0.01, 0.0
    dflux, g = np.zeros(nlevel), np.zeros(nlevel)
    flag_converge = 0
    for its in range(it_max):
        f_vec, flux_net = residual(flux_net_ir, flux_net_ir_layer)
        dflux[:n_total] = f_vec
        beta, temp_old = temp.copy(), temp.copy()
        flux_net_old, flux_net_midpt_old = flux_net_ir.copy(), flux_net_ir_layer.copy()
        sum_1 = np.cumsum(temp[:n_total] ** 2)[-1]                 # the reference sums the first n_total levels
        test = np.fmax.reduce(np.abs(f_vec), initial=0.0)
        f = half_sum_sq(f_vec)
        if test / abs(tidal[0]) < 0.01 * tolf:
            if verbose:
                print(" We are already at a root, tolf , test = ", 0.01 * tolf, ", ", test / abs(tidal[0]))
            if its == 0:                                            # the first evaluation is of this very profile
                return temp, _lapse(temp, pressure), all_profiles, flux_net_ir, flux_net_v, flux_plus_ir[0, :]
            return finish(False)                                    # the trials gave nets only: the fluxes of THIS profile
        if egp_stepmax:
            step_max = 0.005 * max(np.sqrt(sum_1), n_total * 1.0)
        else:
            step_max *= max(np.sqrt(sum_1), n_total * 1.0) * max(0.01, (it_max - its) / it_max)

        # ---- the Jacobian: one perturbed profile per unknown, all in one batch.  `temp` is the running profile the
        # reference rebuilds in place, so a level no zone rewrites keeps what the previous profile left there
        del_t = np.maximum(eps * temp_old[unknown], 3.0)
        profiles = np.empty((n_total, nlevel))
        for k, jm in enumerate(unknown):
            beta[jm] += del_t[k]
            for zone in zones:
                temp[zone[0]:zone[1] + 1] = beta[zone[0]:zone[1] + 1]
                adiabat(temp, zone, beta)
            profiles[k] = temp
            beta[jm] = beta[jm] - del_t[k]
        net_layer_b, net_b = nets(profiles)
        A = np.zeros((nlevel, nlevel))
        rows = np.where(first[None, :], net_b[:, unknown] - flux_net_old[unknown],
                        net_layer_b[:, unknown - 1] - flux_net_midpt_old[unknown - 1])      # (profile, residual)
        A[:n_total, :n_total] = (rows / del_t[:, None]).T
        flux_net_ir_layer, flux_net_ir = net_layer_b[-1], net_b[-1]

        g[:] = 0.0
        for j in range(n_total):                                   # g = A^T f, summed over j in order
            g[:n_total] += A[j, :n_total] * f_vec[j]
        p = np.zeros(nlevel)
        p[:n_total] = -f_vec
        f_old = f
        A, p = mat_sol(A, nlevel, n_total, p)

        norm = np.sqrt(np.cumsum(np.concatenate(([0.0], p[2:n_total] ** 2)))[-1])         # the first two are left out
        if norm > step_max:
            p[:n_total] *= step_max / norm
            dflux[:n_total] = -p[:n_total]
        slope = np.cumsum(g[:n_total] * p[:n_total])[-1]
        test = np.fmax.reduce(np.abs(p[:n_total]) / temp_old[:n_total], initial=0.0)
        alamin = tolx / test
        alam, f2, check = 1.0, f, False
        flag_converge = 0
        while flag_converge == 0:
            for zone in zones:
                n_top, n_strt, _, sh = zone
                temp[n_top:n_strt + 1] = beta[n_top:n_strt + 1] + alam * p[n_top - sh:n_strt + 1 - sh]
                adiabat(temp, zone, None)
            low, high = temp < tmin, temp > tmax                  # the damper
            temp[low], temp[high] = tmin + 0.1, tmax - 0.1
            net_layer_b, net_b = nets(temp[None, :])
            flux_net_ir_layer, flux_net_ir = net_layer_b[0], net_b[0]
            f_vec, flux_net = residual(flux_net_ir, flux_net_ir_layer)
            f = half_sum_sq(f_vec)
            if alam < alamin:
                check = True
                flag_converge, check = check_convergence(f_vec, n_total, tolf, check, f, dflux, tolmin, temp, temp_old, g, tolx)
            elif f <= f_old + alf * alam * slope:
                flag_converge, check = check_convergence(f_vec, n_total, tolf, check, f, dflux, tolmin, temp, temp_old, g, tolx)
            else:                                                  # backtrack: quadratic first, then cubic
                if alam == 1.0:
                    tmplam = -slope / (2 * (f - f_old - slope))
                else:
                    rhs_1 = f - f_old - alam * slope
                    rhs_2 = f2 - f_old - alam2 * slope
                    anr = ((rhs_1 / alam ** 2) - (rhs_2 / alam2 ** 2)) / (alam - alam2)
                    b = (-alam2 * rhs_1 / alam ** 2 + alam * rhs_2 / alam2 ** 2) / (alam - alam2)
                    if anr == 0:
                        tmplam = -slope / (2.0 * b)
                    else:
                        disc = b * b - 3.0 * anr * slope
                        if disc < 0.0:
                            tmplam = 0.5 * alam
                        elif b <= 0.0:
                            tmplam = (-b + np.sqrt(disc)) / (3.0 * anr)
                        else:
                            tmplam = -slope / (b + np.sqrt(disc))
                    if tmplam > 0.5 * alam:
                        tmplam = 0.5 * alam
            if flag_converge not in (1, 2):
                alam2, f2 = alam, f
                alam = max(tmplam, 0.1 * alam)
            if np.isnan(np.sum(temp)):
                flag_converge = 1
                temp = temp_old.copy() + 0.5
                if verbose:
                    print("Got stuck with temp NaN -- so escaping the while loop in tstart")
        if verbose:
            print("Iteration number ", its, ", min , max temp ", temp.min(), temp.max(), ", flux balance ",
                  flux_net[0] / abs(tidal[0]))
        if save_profile == 1:
            all_profiles = np.append(all_profiles, temp_old)
        if flag_converge == 2:
            if verbose:
                print("In t_start: Converged Solution in iterations ", its)
            return finish(False)
    if verbose:
        print("Iterations exceeded it_max ! sorry ")
    return finish(True)


# ---------------------------------------------------------------------------------------------------------------------
# The driver around t_start (reference climate.py: get_kzz :331-493, update_kzz :56-124, update_quench_levels :23-54, profile
# :2926-3249, find_strat :2542-2839, run_chemeq_climate_workflow :217-326, run_diseq_climate_workflow :126-214).  Host code
# on nlevel-sized vectors; the device work is what calculate_atm, t_start and get_fluxes do.  profile and find_strat reach
# those three through this module's names, so a test may replace them.
# ---------------------------------------------------------------------------------------------------------------------
SIGMA_SB = 0.56687e-4                                            # erg cm^-2 s^-1 K^-4, the reference's value


def get_kzz(grav, tidal, flux_net_ir_layer, flux_plus_ir_attop, Adiabat, nstr, Atmosphere, moist=False):
    """Eddy diffusion coefficient (cm^2/s) at every level from mixing-length theory (reference climate.py:331-493).

    The convective heat flux of a layer is the emergent flux minus the radiative net flux there, built from the bottom
    layer (which carries everything) upward and never falling faster than ``1/3 p_i / p_{i+1}`` per layer; it is rescaled so
    that the bottom layer carries ``|tidal[0]|`` and floored at the flux of 5 % of the target effective temperature.  The
    mixing length is the scale height times ``max(0.1, min(1, dtdp / grad_ad))``.  ``kz[-1]`` is appended for the last level.
    Inside the radiative zone(s) (``nstr[0]:nstr[1]`` and, when ``nstr[3] != 0``, ``nstr[3]:nstr[4]``) every value is then
    replaced by the mean over two scale heights either side, clipped to the zone.

    Kept from the reference: the altitude ``z`` is filled up to index ``nlevel - 3`` only, its last element stays 0 (and
    takes part in the nearest-altitude searches); the averages of the lower zone are taken after the upper zone has been
    overwritten; ``grav`` is in m/s^2.  ``moist=True`` is not implemented."""
    if moist:
        raise NotImplementedError("get_kzz: the moist adiabat (moist=True) is not implemented")
    pressure, temp = f64(Atmosphere.p_level), f64(Atmosphere.t_level)
    mmw, dtdp = f64(Atmosphere.mmw_layer), f64(Atmosphere.dtdp)
    tidal, net_layer = f64(tidal), f64(flux_net_ir_layer)
    nstr = [int(x) for x in nstr]
    nlevel = len(temp)
    nz = nlevel - 1
    grav_cgs = grav * 1e2
    r_atmos = 8.3143e7 / mmw
    p_layer = np.sqrt(pressure[1:] * 1e6 * (pressure[:-1] * 1e6))
    t_layer = 0.5 * (temp[1:] + temp[:-1])
    p_layer_bar = np.sqrt(pressure[1:] * pressure[:-1])
    f_sum = np.sum(f64(flux_plus_ir_attop))
    target_teff = (abs(tidal[0]) / SIGMA_SB) ** 0.25
    flx_min = SIGMA_SB * ((target_teff * 0.05) ** 4)

    chf = np.zeros(tidal.shape)
    chf[nz - 1] = f_sum                                           # the bottom layer: all convective
    for iz in range(nz - 2, -1, -1):
        chf[iz] = max(f_sum - net_layer[iz], (1.0 / 3.0) * p_layer[iz] / p_layer[iz + 1] * chf[iz + 1])
    ratio = abs(tidal[0]) / chf[nz - 1]
    chf[:nz] = np.maximum(chf[:nz] * ratio, flx_min)

    grad_x = np.array([did_grad_cp(t, p, Adiabat)[0] for t, p in zip(t_layer, p_layer_bar)])     # per layer, as the reference
    lapse_ratio = np.minimum(1.0, dtdp / grad_x)
    rho_atmos = p_layer / (r_atmos * t_layer)
    c_p = (7.0 / 2.0) * r_atmos
    scale_h = r_atmos * t_layer / grav_cgs
    mixl = np.maximum(0.1, lapse_ratio) * scale_h
    kz = (1.0 / 3.0) * scale_h * (mixl / scale_h) ** (4.0 / 3.0) * ((r_atmos * chf[:-1]) / (rho_atmos * c_p)) ** (1.0 / 3.0)
    kz = np.append(kz, kz[-1])

    dz = scale_h[1:] * np.log((p_layer[:-1] / 1e6) / (p_layer[1:] / 1e6))
    z = np.zeros(nlevel - 1)
    z[:nlevel - 2] = np.cumsum(dz[:nlevel - 2])                  # z[nlevel-2] stays 0, as in the reference

    def zone_means(lo, hi):
        out = []
        for i in range(lo, hi):
            above = abs(i - int(np.abs(z - (z[i] + 2 * scale_h[i])).argmin()))
            below = abs(i - int(np.abs(z - (z[i] - 2 * scale_h[i])).argmin()))
            out.append(np.mean(kz[max(lo, i - above):min(hi, i + below)]))
        return np.array(out)
    kz[nstr[0]:nstr[1]] = zone_means(nstr[0], nstr[1])
    if nstr[3] != 0:
        kz[nstr[3]:nstr[4]] = zone_means(nstr[3], nstr[4])
    return kz


def update_kzz(grav, tidal, AdiabatBundle, nstr, Atmosphere, OpacityWEd=None, OpacityNoEd=None, ScatteringPhase=None,
               Disco=None, Opagrid=None, F0PI=None, OpacityWEd_clear=None, OpacityNoEd_clear=None, flux_net_ir_layer=None,
               flux_plus_ir_attop=None, moist=False, do_holes=False, fhole=None, verbose=True, _fluxes=None):
    """``get_kzz`` with the fluxes handed in, or -- when neither ``flux_net_ir_layer`` nor ``flux_plus_ir_attop`` is given --
    with those of one thermal ``get_fluxes`` call at ``Atmosphere`` (reference climate.py:56-124).  ``_fluxes``: as in
    ``t_start``; its first callable stands in for ``get_fluxes``."""
    if verbose:
        print("update_kzz: mixing-length kzz profile")
    if flux_plus_ir_attop is None and flux_net_ir_layer is None:
        single = get_fluxes if _fluxes is None else _fluxes[0]
        holes = {}
        if do_holes:
            holes = dict(do_holes=True, fhole=fhole, hole_OpacityWEd=OpacityWEd_clear, hole_OpacityNoEd=OpacityNoEd_clear)
        out = single(Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Opagrid, F0PI, False, True, **holes)
        flux_net_ir_layer, flux_plus_ir_attop = out[4], out[6][0, :]
    return get_kzz(grav, tidal, flux_net_ir_layer, flux_plus_ir_attop, AdiabatBundle, nstr, Atmosphere, moist=moist)


def update_quench_levels(bundle, Atmosphere, kz, grav, verbose=False):
    """Quench levels of the bundle's current (equilibrium) chemistry (reference climate.py:23-54): ``get_quench_levels`` with
    the metallicity ``bundle.inputs['atmosphere']['mh']`` (1, with the reference's warning, when it was not set).  PH3 is
    quenched only when ``H2``, ``H2O`` and ``PH3`` are all columns of the profile."""
    prof = bundle.inputs["atmosphere"]["profile"]
    if all(m in prof.keys() for m in ("H2", "H2O", "PH3")):
        H2O, H2, PH3 = np.asarray(prof["H2O"], dtype=float), np.asarray(prof["H2"], dtype=float), True
    else:
        H2O, H2, PH3 = None, None, False
    mh_linear = bundle.inputs["atmosphere"].get("mh", None)
    if mh_linear is None:
        print("User warning: mh was not explicitly set so we are assuming no metallicity dependence (e.g., M/H=1xSolar) for "
              "the quench approximations published in Zahnle and Marley 2014")
        mh_linear = 1
    quench_levels, _ = get_quench_levels(Atmosphere, kz, grav, mh_linear, PH3=PH3, H2O=H2O, H2=H2)
    if verbose:
        print("Computed quenched levels at", quench_levels)
    return quench_levels


def profile(bundle, nofczns, nstr, temp, pressure, AdiabatBundle, opacityclass, grav, rfaci, rfacv, tidal, Opagrid,
            CloudParameters, save_profile, all_profiles, all_opd, convergence_criteria, final, flux_net_ir_layer=None,
            flux_plus_ir_attop=None, first_call_ever=False, verbose=True, moist=None, save_kzz=False,
            self_consistent_kzz=True, diseq=False, all_kzz=[], _fluxes=None):
    """One outer step of the climate solve with the convective zones ``nstr`` held fixed (reference ``climate.profile``,
    climate.py:2926-3249; same positional arguments): lay the adiabat through every convective zone of ``temp``, refresh the
    chemistry and the opacities, then call ``t_start`` up to ``convergence_criteria.itmx`` times, each from the profile the
    last one returned, until the mean temperature change falls below ``convt``.  Returns the reference's list
    ``[conv_flag, pressure, temp, dtdp, CloudParameters, cld_out, flux_net_ir_layer, flux_net_v_layer, flux_plus_ir_attop,
    all_profiles, all_opd, all_kzz]`` (``cld_out`` is NaN: no clouds).

    Kept from the reference:
    * ``egp_stepmax`` (the small fixed step cap of ``t_start``) when the coldest level of the ENTRY profile is <= 250 K;
    * the adiabat uses ``did_grad_cp`` at the level above and ``sqrt(p[j-1] p[j])``, level by level;
    * ``bundle.add_pt``, ``bundle.premix_atmosphere`` and ``calculate_atm`` run once before the loop; inside it only the
      chemistry of the bundle follows the new profile -- cloud-free equilibrium chemistry needs no refresh, so every
      ``t_start`` call of one ``profile`` call sees the SAME opacity planes (the DeviceArrays of ``calculate_atm``, handed on
      as they are).  With ``diseq`` the planes ARE refreshed, before the loop and after every ``t_start`` call (below);
    * each ``t_start`` call starts from the temperatures the previous one returned (the reference's ``t_start`` works in
      ``Atmosphere.t_level`` itself), and ``Atmosphere.dtdp`` stays that of the entry profile, which is what ``get_kzz`` reads;
    * the kzz profile is computed with ``save_kzz`` or with ``self_consistent_kzz and diseq`` (before the loop from a fresh
      thermal ``get_fluxes`` call, inside it from the fluxes ``t_start`` returned); the one before the loop is booked in
      ``bundle.inputs['atmosphere']['kzz']['sc_kzz']``; ``all_kzz`` collects them only with ``save_kzz``;
    * converged means ``iii > 0 and sum|dT| / (1.5 nlevel) < convt`` (the cloud term ``taudif = 0 < 0.1`` always holds); the
      reference then sets ``itmx`` of its local copy of the criteria, which nobody reads;
    * with ``CloudParameters.cloudy`` false ``do_holes`` is false whatever ``bundle.inputs['clouds']`` says, so the hole
      planes ``calculate_atm`` may return are not used;
    * ``flux_net_ir_layer`` / ``flux_plus_ir_attop`` / ``first_call_ever`` are accepted and not read.

    ``diseq=True`` (the quench approximation, climate.py:3083-3124 and :3153-3209): before the loop and after every ``t_start``
    call the equilibrium chemistry of the new profile (``premix_atmosphere(quench_levels=None)``) is followed by
    ``update_kzz`` (self-consistent kzz) or the bundle's ``['kzz']['constant_kzz']`` (``self_consistent_kzz=False``),
    ``update_quench_levels``, ``premix_atmosphere(quench_levels=...)`` and a fresh ``calculate_atm``, whose planes replace the
    old DeviceArrays (they are freed with their last reference: device memory stays flat).  Before the loop that is a
    second ``calculate_atm`` and the kzz comes from the planes of the first, the equilibrium ones.  Inside the loop the
    ``Atmosphere`` handed to ``update_kzz`` / ``update_quench_levels`` is that of the last ``calculate_atm`` with the new
    temperatures: its ``dtdp``, ``mmw_layer`` and ``scale_height`` are the older ones, as in the reference, whose ``t_start``
    writes into ``Atmosphere.t_level``.  The bundle must have ``chem_params['quench']`` set (``atmosphere(quench=True)``):
    without it ``premix_atmosphere`` ignores the levels and the run would silently be the equilibrium one with the cost of
    the refreshes, which is refused.

    ``temp`` is not modified (the reference lays the adiabat into the caller's array; its callers use the returned one).
    Not implemented, each a ``NotImplementedError``: ``CloudParameters.cloudy`` (virga), ``moist=True`` (the moist
    adiabat), a photochem ``chem_method``.

    ``_fluxes``: handed to every ``t_start`` call and to ``update_kzz``."""
    if "photochem" in str(bundle.inputs["approx"].get("chem_method", None)):
        raise NotImplementedError("profile: chem_method='photochem' needs the photochem package, which is not part of this "
                                  "package")
    if diseq and not bundle.inputs["approx"].get("chem_params", {}).get("quench", False):
        raise NotImplementedError("profile: diseq=True without chem_params['quench'] is not implemented: premix_atmosphere "
                                  "would ignore the quench levels and the run would be the equilibrium one; call "
                                  "atmosphere(quench=True) after inputs_climate")
    if CloudParameters.cloudy:
        raise NotImplementedError("profile: CloudParameters.cloudy needs virga (update_clouds), which is not implemented")
    if moist:
        raise NotImplementedError("profile: the moist adiabat (moist=True) is not implemented")
    F0PI = opacityclass.relative_flux
    convt, itmx = convergence_criteria.convt, int(convergence_criteria.itmx)
    do_holes, fhole = False, None                                 # climate.py:3020-3022: no clouds, no holes
    temp, pressure = np.array(temp, dtype=np.float64), f64(pressure)
    nstr = [int(x) for x in nstr]
    egp_stepmax = bool(np.min(temp) <= 250)
    conv_flag = 0
    sc_kzz_and_diseq = bool(self_consistent_kzz and diseq)
    do_kzz_calc = sc_kzz_and_diseq or bool(save_kzz)              # climate.py:3006-3012, without clouds
    kz_chem = None
    if diseq and not self_consistent_kzz:
        kz_chem = bundle.inputs["atmosphere"]["kzz"].get("constant_kzz")

    for nb in range(0, 3 * int(nofczns), 3):                      # the adiabat through every convective zone
        for j1 in range(nstr[nb + 1] + 1, nstr[nb + 2] + 2):
            grad_x, _ = did_grad_cp(temp[j1 - 1], np.sqrt(pressure[j1 - 1] * pressure[j1]), AdiabatBundle)
            temp[j1] = np.exp(np.log(temp[j1 - 1]) + grad_x * (np.log(pressure[j1]) - np.log(pressure[j1 - 1])))
    temp_old = temp.copy()
    if save_profile == 1:
        all_profiles = np.append(all_profiles, temp_old)

    bundle.add_pt(temp, pressure)
    bundle.premix_atmosphere(opa=opacityclass, quench_levels=None, verbose=verbose)
    OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Atmosphere, _ = calculate_atm(bundle, opacityclass)
    if do_kzz_calc:
        kz = update_kzz(grav, tidal, AdiabatBundle, nstr, Atmosphere, OpacityWEd=OpacityWEd, OpacityNoEd=OpacityNoEd,
                        ScatteringPhase=ScatteringPhase, Disco=Disco, Opagrid=Opagrid, F0PI=F0PI, moist=False,
                        do_holes=do_holes, fhole=fhole, verbose=verbose, _fluxes=_fluxes)
        bundle.inputs["atmosphere"].setdefault("kzz", {})["sc_kzz"] = kz
        if save_kzz:
            all_kzz = np.append(all_kzz, kz)
        if sc_kzz_and_diseq:
            kz_chem = kz

    def quench_and_refresh(Atmosphere):
        """Quench the bundle's equilibrium chemistry at the levels of `Atmosphere` and `kz_chem`; the new planes."""
        quench_levels = update_quench_levels(bundle, Atmosphere, kz_chem, grav, verbose=verbose)
        bundle.premix_atmosphere(opa=opacityclass, quench_levels=quench_levels, verbose=verbose)
        return calculate_atm(bundle, opacityclass)[:5]
    if diseq:
        OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Atmosphere = quench_and_refresh(Atmosphere)

    RETURNS = None
    dtdp = Atmosphere.dtdp
    for iii in range(itmx):
        Atmosphere = Atmosphere._replace(t_level=temp)            # the reference's t_start left its result in this array
        temp, dtdp, all_profiles, flux_net_ir_layer, flux_net_v_layer, flux_plus_ir_attop = t_start(
            nofczns, nstr, convergence_criteria, rfaci, rfacv, tidal, Atmosphere, OpacityWEd, OpacityNoEd, ScatteringPhase,
            Disco, Opagrid, AdiabatBundle, F0PI, save_profile, all_profiles, verbose=verbose, moist=False,
            egp_stepmax=egp_stepmax, _fluxes=_fluxes)
        bundle.add_pt(temp, pressure)
        bundle.premix_atmosphere(opa=opacityclass, quench_levels=None, verbose=verbose)
        if do_kzz_calc:
            kz = update_kzz(grav, tidal, AdiabatBundle, nstr, Atmosphere._replace(t_level=temp),
                            flux_net_ir_layer=flux_net_ir_layer, flux_plus_ir_attop=flux_plus_ir_attop, moist=False,
                            do_holes=do_holes, fhole=fhole, verbose=verbose)
            if save_kzz:
                all_kzz = np.append(all_kzz, kz)
            if sc_kzz_and_diseq:
                kz_chem = kz
        if diseq:
            OpacityWEd, OpacityNoEd, ScatteringPhase, Disco, Atmosphere = quench_and_refresh(
                Atmosphere._replace(t_level=temp))
        RETURNS = [conv_flag, pressure, temp, dtdp, CloudParameters, np.nan, flux_net_ir_layer, flux_net_v_layer,
                   flux_plus_ir_attop, all_profiles, all_opd, all_kzz]
        ert = np.sum(np.abs(temp - temp_old)) / (float(len(temp)) * 1.5)
        temp_old = temp.copy()
        if iii > 0 and ert < convt:
            if verbose:
                print("profile: converged at outer iteration", iii)
            RETURNS[0] = 1
            return RETURNS
        if verbose:
            print("profile: outer iteration", iii, "coldest level", min(temp))
    if RETURNS is None:
        raise ValueError("profile: convergence_criteria.itmx must be at least 1")
    if verbose:
        print("profile: itmx reached without convergence")
    return RETURNS


def find_strat(bundle, nofczns, nstr, temp, pressure, dtdp, AdiabatBundle, opacityclass, grav, rfaci, rfacv, tidal, Opagrid,
               CloudParameters, save_profile, all_profiles, all_opd, flux_net_ir_layer, flux_plus_ir_attop, verbose=1,
               moist=None, save_kzz=False, self_consistent_kzz=True, diseq=False, all_kzz=[], _fluxes=None):
    """Find the convective zones (reference ``climate.find_strat``, climate.py:2542-2839; same positional arguments): grow
    the convective zone upward while the layer above it is steeper than 0.98 of the adiabat, look for a detached second
    zone, grow both, merge them when they meet, calling ``profile`` with the criteria ``(8, 5, 5.0, 3.0, 7.0)`` after every
    change and with ``(10, 6, 2.0, 2.0, 3.5)`` and ``final=True`` at the end.  Returns ``profile_flag, pressure, temp, dtdp,
    nstr, flux_net_ir_layer, flux_net_v_layer, flux_plus_ir_attop, chem, cld_out, all_profiles, all_opd, all_kzz``.

    ``nstr`` must be a list (or array) of six integers and IS MODIFIED IN PLACE, as the reference does; the returned one is
    the same object.

    Kept from the reference:
    * ``subad = 0.98``, and the search for a second zone ends at level ``ifirst = 9``;
    * the adiabatic gradient ``grad_x`` is computed ONCE, at the entry profile, and never refreshed, while ``dtdp`` follows
      every ``profile`` call (the ``dtdp`` argument itself is replaced at once by that of ``calculate_atm``);
    * the first zone grows by 2 levels while ``dtdp / grad_x > 1.8``, else by 1; it may not pass level 5
      (later, in the grow phase, level 3): ``ValueError``;
    * the second zone is put at the FIRST layer from below, ``nstr[1] - 1`` down to 9, whose excess over the adiabat is at
      least 2 % (the loop breaks there; it does not look for the largest);
    * ``nstr[3] = i_max``, not ``i_max + 1``; ``nstr[3] >= nstr[4]`` raises "Overlap happened !";
    * in the grow phase the upper zone grows up when its excess is the larger one (or one zone is left), else it grows down
      towards the lower zone; the lower zone then grows up; when ``nstr[2] == nstr[4]`` the two become one zone and the
      phase runs again."""
    criteria = convergence_criteriaT(it_max=8, itmx=5, conv=5.0, convt=3.0, x_max_mult=7.0)
    subad, ifirst = 0.98, 10 - 1
    state = dict(flux_net_ir_layer=flux_net_ir_layer, flux_plus_ir_attop=flux_plus_ir_attop, all_profiles=all_profiles,
                 all_opd=all_opd, all_kzz=all_kzz, CloudParameters=CloudParameters, temp=temp, pressure=pressure)

    def step(nofczns, criteria, final):
        out = profile(bundle, nofczns, nstr, state["temp"], state["pressure"], AdiabatBundle, opacityclass, grav, rfaci,
                      rfacv, tidal, Opagrid, state["CloudParameters"], save_profile, state["all_profiles"],
                      state["all_opd"], criteria, final, flux_net_ir_layer=state["flux_net_ir_layer"],
                      flux_plus_ir_attop=state["flux_plus_ir_attop"], verbose=verbose, moist=moist, save_kzz=save_kzz,
                      self_consistent_kzz=self_consistent_kzz, diseq=diseq, all_kzz=state["all_kzz"], _fluxes=_fluxes)
        (state["flag"], state["pressure"], state["temp"], dtdp, state["CloudParameters"], state["cld_out"],
         state["flux_net_ir_layer"], state["flux_net_v_layer"], state["flux_plus_ir_attop"], state["all_profiles"],
         state["all_opd"], state["all_kzz"]) = out
        return dtdp

    bundle.add_pt(temp, pressure)
    bundle.premix_atmosphere(opacityclass, verbose=verbose)
    Atmosphere = calculate_atm(bundle, opacityclass, only_atmosphere=True)
    dtdp = Atmosphere.dtdp
    grad_x, _ = convec(temp, pressure, AdiabatBundle, Atmosphere, moist=moist)          # once: never refreshed

    while dtdp[nstr[1] - 1] >= subad * grad_x[nstr[1] - 1]:
        ngrow = 2 if dtdp[nstr[1] - 1] / grad_x[nstr[1] - 1] > 1.8 else 1
        if verbose and ngrow == 2:
            print("find_strat: lapse rate above 1.8 x adiabatic, growing by two levels")
        growup(1, nstr, ngrow)
        if nstr[1] < 5:
            raise ValueError("Convection zone grew to Top of atmosphere, Need to Stop")
        dtdp = step(nofczns, criteria, False)

    dt_max, i_max = 0.0, 0
    for i in range(nstr[1] - 1, ifirst - 1, -1):                  # the first super-adiabatic layer from below: `break`
        add = dtdp[i] - grad_x[i]
        if add > dt_max and add / grad_x[i] >= 0.02:
            dt_max, i_max = add, i
            break

    if not (i_max == 0 or dt_max / grad_x[i_max] < 0.02):
        if verbose:
            print("find_strat: second convective zone at layer", i_max, "zones before", nstr)
        nofczns = 2
        nstr[4], nstr[5] = nstr[1], nstr[2]
        nstr[1] = nstr[2] = nstr[3] = i_max                       # nstr[3]: i_max, not i_max + 1
        if nstr[3] >= nstr[4]:
            raise ValueError("Overlap happened !")
        dtdp = step(nofczns, criteria, False)

        def merge():
            nstr[2], nstr[3] = nstr[5], 0
            return 1, 1
        i_change = 1
        while i_change == 1:
            if verbose:
                print("find_strat: grow phase")
            i_change = 0
            d1, d2, c1, c2 = dtdp[nstr[1] - 1], dtdp[nstr[3]], grad_x[nstr[1] - 1], grad_x[nstr[3]]
            while d1 > subad * c1 or d2 > subad * c2:
                if (d1 - c1) >= (d2 - c2) or nofczns == 1:
                    growup(1, nstr, 1)
                    if nstr[1] < 3:
                        raise ValueError("Convection zone grew to Top of atmosphere, Need to Stop")
                else:
                    growdown(1, nstr, 1)
                    if nstr[2] == nstr[4]:                        # the two zones met: one zone
                        nofczns, i_change = merge()
                if verbose:
                    print(nstr)
                dtdp = step(nofczns, criteria, False)
                d1, d2, c1, c2 = dtdp[nstr[1] - 1], dtdp[nstr[3]], grad_x[nstr[1] - 1], grad_x[nstr[3]]
            while dtdp[nstr[4] - 1] >= subad * grad_x[nstr[4] - 1] and nofczns > 1:      # the lower zone
                growup(2, nstr, 1)
                if nstr[2] == nstr[4]:
                    nofczns, i_change = merge()
                if verbose:
                    print(nstr)
                dtdp = step(nofczns, criteria, False)

    criteria = convergence_criteriaT(10, 6, 2.0, 2.0, 7.0 / 2.0)
    if verbose:
        print("find_strat: final profile call with zones", nstr)
    dtdp = step(nofczns, criteria, True)
    if verbose:
        print("find_strat: converged" if state["flag"] == 1 else "find_strat: ended without convergence")
    chem = bundle.inputs["atmosphere"]["profile"]
    return (state["flag"], state["pressure"], state["temp"], dtdp, nstr, state["flux_net_ir_layer"],
            state["flux_net_v_layer"], state["flux_plus_ir_attop"], chem, state["cld_out"], state["all_profiles"],
            state["all_opd"], state["all_kzz"])


def run_chemeq_climate_workflow(bundle, nofczns, nstr, temp, pressure, AdiabatBundle, opacityclass, grav, rfaci, rfacv, tidal,
                                Opagrid, CloudParameters, save_profile, all_profiles, all_opd, verbose=True, moist=None,
                                save_kzz=True, self_consistent_kzz=True, _fluxes=None):
    """The equilibrium-chemistry climate solve (reference climate.py:217-326): ``profile`` with the loose criteria
    ``(10, 7, 10.0, 5.0, 7.0)``, again with ``(7, 5, 5.0, 4.0, 7.0)``, then ``find_strat``.  Returns ``find_strat``'s 13 values.
    As in the reference ``find_strat`` is called WITHOUT ``save_kzz`` (it keeps its default, False): kzz profiles are
    collected during the two ``profile`` calls only.  ``nstr`` is modified in place."""
    common = (AdiabatBundle, opacityclass, grav, rfaci, rfacv, tidal, Opagrid)
    out = profile(bundle, nofczns, nstr, temp, pressure, *common, CloudParameters, save_profile, all_profiles, all_opd,
                  convergence_criteriaT(10, 7, 10.0, 5.0, 7.0), False, first_call_ever=True, verbose=verbose, moist=moist,
                  save_kzz=save_kzz, self_consistent_kzz=self_consistent_kzz, _fluxes=_fluxes)
    _, pressure, temperature, dtdp, CloudParameters, _, net_layer, _, plus_top, all_profiles, all_opd, all_kzz = out
    out = profile(bundle, nofczns, nstr, temperature, pressure, *common, CloudParameters, save_profile, all_profiles,
                  all_opd, convergence_criteriaT(7, 5, 5.0, 4.0, 7.0), False, flux_net_ir_layer=net_layer,
                  flux_plus_ir_attop=plus_top, verbose=verbose, moist=moist, save_kzz=save_kzz, all_kzz=all_kzz,
                  self_consistent_kzz=self_consistent_kzz, _fluxes=_fluxes)
    _, pressure, temperature, dtdp, CloudParameters, _, net_layer, _, plus_top, all_profiles, all_opd, all_kzz = out
    return find_strat(bundle, nofczns, nstr, temperature, pressure, dtdp, *common, CloudParameters, save_profile,
                      all_profiles, all_opd, net_layer, plus_top, verbose=verbose, moist=moist,
                      self_consistent_kzz=self_consistent_kzz, all_kzz=all_kzz, _fluxes=_fluxes)


def run_diseq_climate_workflow(bundle, nofczns, nstr, temp, pressure, AdiabatBundle, opacityclass, grav, rfaci, rfacv, tidal,
                               Opagrid, CloudParameters, save_profile, all_profiles, all_opd, verbose=True, moist=None,
                               save_kzz=False, self_consistent_kzz=True, _fluxes=None):
    """The climate solve with quench ("disequilibrium") chemistry (reference climate.py:126-214): one ``profile`` call with
    the criteria ``(10, 7, 5.0, 4.0, 7.0)``, then ``find_strat``, both with ``diseq=True`` and -- unlike the equilibrium
    workflow -- both with ``save_kzz``.  Returns ``find_strat``'s 13 values; ``nstr`` is modified in place."""
    common = (AdiabatBundle, opacityclass, grav, rfaci, rfacv, tidal, Opagrid)
    out = profile(bundle, nofczns, nstr, temp, pressure, *common, CloudParameters, save_profile, all_profiles, all_opd,
                  convergence_criteriaT(it_max=10, itmx=7, conv=5.0, convt=4.0, x_max_mult=7.0), False, flux_net_ir_layer=None,
                  flux_plus_ir_attop=None, first_call_ever=False, verbose=verbose, moist=moist, save_kzz=save_kzz,
                  self_consistent_kzz=self_consistent_kzz, diseq=True, _fluxes=_fluxes)
    _, pressure, temperature, dtdp, CloudParameters, _, net_layer, _, plus_top, all_profiles, all_opd, all_kzz = out
    return find_strat(bundle, nofczns, nstr, temperature, pressure, dtdp, *common, CloudParameters, save_profile,
                      all_profiles, all_opd, net_layer, plus_top, verbose=verbose, moist=moist, save_kzz=save_kzz,
                      self_consistent_kzz=self_consistent_kzz, diseq=True, all_kzz=all_kzz, _fluxes=_fluxes)
