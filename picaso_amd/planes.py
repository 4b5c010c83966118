"""Which of ``compute_opacity``'s 13 planes a spectrum writes, and what its solvers read in place of the others.

Every spectrum path -- ``spectrum.Spectrum`` (call by call, batch, wavelength blocks) and the one-call driver
(``onecall`` / ``driver.BlockTable``) -- takes its plane set from ``choose_1d`` / ``choose_3d`` and its solver inputs from
``views``, so the paths write the same planes and read the same buffers: same bits.  Host only; the predicates of what the
kernels re-derive (``resident.reflected_can_derive*``) need the library, not a GPU.
"""
from typing import NamedTuple

import numpy as np

OUT_NAMES = ("dtau", "tau", "w0", "cosb", "ftau_cld", "ftau_ray", "gcos2", "dtau_og", "tau_og", "w0_og", "cosb_og",
             "w0_no_raman", "f_deltaM")                   # compute_opacity / picaso_compute_opacity_ck_dev order
REFLECTED_PLANES = ("dtau", "tau", "w0", "cosb", "gcos2", "ftau_cld", "ftau_ray", "dtau_og", "tau_og", "w0_og",
                    "cosb_og")                            # the Toon reflected-light kernels
SH_PLANES = ("dtau", "tau", "w0", "cosb", "ftau_cld", "ftau_ray", "f_deltaM", "dtau_og", "tau_og", "w0_og",
             "cosb_og")                                   # the SH reflected-light kernels
SH_READS = ("dtau", "w0", "cosb_og", "ftau_cld", "ftau_ray", "f_deltaM", "dtau_og", "w0_og")    # ... when levels are derived
DERIVED = ("tau", "tau_og", "gcos2")                      # running sums and 0.5 ftau_ray: re-derived by the Toon kernels
THERMAL = ("dtau_og", "w0_no_raman", "cosb_og")           # what the Toon thermal kernels read (dtau, w0, cosb)
THERMAL_SH = ("dtau", "w0", "cosb_og")                    # ... and get_thermal_SH


class Choice(NamedTuple):
    """``want``: the planes compute_opacity writes (None: all 13).  ``lean``: Toon, cloud-free -- the others are aliases
    and constants (``views``).  ``derive``: the Toon reflected kernel re-derives ``DERIVED`` (cloud-free: all but dtau and
    w0).  ``sh_lean``: SH, cloud-free, default forms -- dtau and w0 are all the launch reads.  ``sh_top``: the cloud-free
    layers above an SH cloud deck.  ``thermal``: the (dtau, w0, cosb) names the thermal leg reads -- 1-D: in the map
    ``views`` returns; 3-D: planes as written, cosb None = not read -- or None without a thermal leg."""
    want: frozenset = None
    lean: bool = False
    derive: bool = False
    sh_lean: bool = False
    sh_top: int = 0
    thermal: tuple = None


def cloud_free_top(inp, nlayer):
    """Number of layers above the cloud deck: the first layer whose cloud profile rows hold any optical depth or any
    asymmetry (COSB is the cloud's g0 itself, optics.py:338, so a g0 without optical depth still delta-scales the layer).
    Read off the profile AS GIVEN (linear regridding keeps a zero row zero); tables larger than 2e5 numbers are not
    scanned (0: no statement) -- the scan would cost more than it saves."""
    prof = inp["clouds"]["profile"]
    if prof is None:
        return nlayer
    busy = np.zeros(nlayer, dtype=bool)
    for k in ("opd", "g0"):
        v = np.asarray(prof[k], dtype=np.float64)
        if v.ndim == 0:
            return 0 if v != 0 else nlayer
        if v.size > 200000 or v.size % nlayer:
            return 0
        busy |= (v.reshape(nlayer, -1) != 0).any(axis=1)
    return int(np.argmax(busy)) if busy.any() else nlayer


def choose_1d(inp, atm, nwno, ngauss, calculation, full_output=False, all_planes=False):
    """The plane set of a 1-D spectrum: ``inp`` = the case's inputs, ``atm`` its ATMSETUP (sizes, ``cloud_free``,
    ``rayleigh_molecules``, ``get_lvl_flux``), ``nwno`` the columns of one Gauss point.

    Only the planes the requested legs read are written (Toon: 11 for reflected light, 3 for thermal emission, 1 for
    transmission; the SH solvers take the whole set).  ``derive``: tau, tau_og (running sums) and gcos2 (0.5 ftau_ray) are
    not written where the reflected launch re-derives them exactly (resident.reflected_can_derive).  ``lean``: a cloud-free
    atmosphere (no cloud profile, no test mode) -- most of the 13 planes are copies of others or constants (cosb = cosb_og
    = ftau_cld = 0, ftau_ray = 1, gcos2 = 0.5, and with cosb = 0 the delta-scaling is the identity: dtau_og = dtau, tau_og
    = tau, w0_og = w0), so only dtau, tau and w0 are written (0.26 -> 0.09 ms of mixing at 1e5 x 90); w0_no_raman equals
    w0 when the Raman factor is the constant 0.99999 (raman='none').  ``sh_lean``: SH with the reference's default forms,
    same atmosphere: dtau and w0.  ``sh_top``: a cloud deck -- the layers above it go through the cloud-free SH kernel; a
    cloudy SH spectrum with the default options leaves out the level planes (running products in the kernel).
    Correlated-k tables (Toon), patchy clouds, test modes and ``all_planes`` take the full set."""
    from . import resident                                # (resident takes its plane names from here)
    approx = inp["approx"]
    common, toon, geom = approx["rt_params"]["common"], approx["rt_params"]["toon"], inp["disco"]
    is_sh = approx["rt_method"] == "SH"
    do_r, do_t = "reflected" in calculation, "thermal" in calculation
    holes = bool(inp["clouds"].get("do_holes", False)) and not is_sh        # (SH ignores patchy clouds)
    plain = ngauss == 1 and inp["test_mode"] is None and not holes and not all_planes
    rayleigh = len(getattr(atm, "rayleigh_molecules", [])) > 0
    cloud_free = bool(getattr(atm, "cloud_free", False))
    frac_c = common["TTHG_params"]["fraction"][2]
    if is_sh:
        sh = approx["rt_params"]["SH"]
        forms = (common["stream"], sh["w_single_form"], sh["w_multi_form"], sh["psingle_form"], sh["w_single_rayleigh"],
                 sh["w_multi_rayleigh"], sh["psingle_rayleigh"], frac_c, sh["single_form"])
        thermal = THERMAL_SH if do_t else None
        if (plain and cloud_free and rayleigh and not full_output
                and resident.reflected_SH_can_derive(*forms, 1 if sh["calculate_fluxes"] else 0)):
            return Choice(frozenset(("dtau", "w0")), sh_lean=True, thermal=thermal)
        # (every wavelength block of a sharded spectrum reads the same profile, hence the same statement)
        top = cloud_free_top(inp, atm.c.nlayer) if (inp["test_mode"] is None and rayleigh and not all_planes) else 0
        # the level planes tau / tau_og are running sums: the default-options launch carries the beam exponentials as
        # running products instead of reading them, and cosb, gcos2, w0_no_raman are read by no SH solver
        levels = (not all_planes and not full_output and resident.reflected_SH_can_derive_levels(
            atm.c.nlevel, nwno * ngauss, *forms, 1 if (sh["calculate_fluxes"] and ngauss == 1) else 0))
        return Choice(frozenset(SH_READS) if levels else None, sh_top=top, thermal=thermal)
    derive = (plain and do_r and not full_output
              and resident.reflected_can_derive(atm.c.nlevel, nwno, geom["num_gangle"], geom["num_tangle"], geom["ubar0"],
                                                geom["ubar1"], geom["cos_theta"], toon["single_phase"],
                                                toon["multi_phase"], frac_c, toon["toon_coefficients"], atm.get_lvl_flux))
    lean = plain and cloud_free and rayleigh
    want = set()
    if lean:
        if do_r:
            want |= {"dtau", "w0"} if derive else {"dtau", "tau", "w0"}
        if do_t:
            want |= {"dtau", "w0" if (common["raman"] == 2 and do_r) else "w0_no_raman"}
    else:
        if do_r:
            want |= set(REFLECTED_PLANES) - (set(DERIVED) if derive else set())
        if do_t:
            want |= set(THERMAL)
    if "transmission" in calculation:
        want.add("dtau" if lean else "dtau_og")
    if not want:        # a calculation that names no leg (full_output of the set-up alone): one plane, no leg reads it
        want = {"dtau" if lean else "dtau_og"}
    return Choice(frozenset(want), lean=lean, derive=derive, thermal=THERMAL if do_t else None)


def choose_3d(inp, calculation, all_planes=False):
    """The plane set of a 3-D spectrum (Toon; every plane is nfacets x 9 MB at 12 500 wavelengths x 90 layers).  The level
    planes and gcos2 are always re-derived in the solvers: the reflected kernel takes 8 planes instead of 11.  Without
    cloud (and outside the test modes) cosb = cosb_og = ftau_cld = 0, ftau_ray = 1 and the delta-scaling is the identity,
    which leaves dtau and w0 -- and w0_no_raman equals w0 for raman='none'.  ``all_planes`` writes the full set."""
    clear = inp["clouds"].get("profile_3d") is None and inp["test_mode"] is None and not all_planes
    do_r, do_t = "reflected" in calculation, "thermal" in calculation
    want, thermal = set(), None
    if do_r:
        if clear:
            want |= {"dtau", "w0"}
        else:
            want |= set(REFLECTED_PLANES) - (set() if all_planes else set(DERIVED))
    if do_t:
        raman = inp["approx"]["rt_params"]["common"]["raman"]
        thermal = ("dtau", "w0" if (raman == 2 and do_r) else "w0_no_raman", None) if clear else THERMAL
        want |= {k for k in thermal if k is not None}
    return Choice(frozenset(want), thermal=thermal)


def views(choice, written, constants):
    """What the 1-D solvers read: ``(legs, refl)``, the name -> buffer maps of every leg and of the reflected-light kernel.
    ``written``: the planes compute_opacity wrote; ``constants()``: resident planes of 0, 1 and 0.5 of the same shape.
    A cloud-free atmosphere (``lean`` / ``sh_lean``) gets the same buffer under several names plus the constants -- same
    values, hence the same bits, as the full set; the reflected kernel that re-derives gets dtau and w0 alone."""
    legs = dict(written)
    if not (choice.lean or choice.sh_lean):
        return legs, legs
    zero, one, half = constants()
    legs.update(dtau_og=legs["dtau"], cosb_og=zero)       # without cloud nothing is delta-scaled
    if choice.sh_lean or choice.derive:
        refl = {"dtau": legs["dtau"], "w0": legs["w0"]}
    else:
        refl = legs
        legs.update(cosb=zero, ftau_cld=zero, ftau_ray=one, gcos2=half)
        if "tau" in legs:
            legs.update(tau_og=legs["tau"], w0_og=legs["w0"])
    if choice.lean and choice.thermal and "w0_no_raman" not in legs:
        legs["w0_no_raman"] = legs["w0"]                  # raman='none': the Raman factor is the constant 0.99999
    return legs, refl
