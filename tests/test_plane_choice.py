"""planes.choose_1d / choose_3d / views -- which of compute_opacity's 13 planes a spectrum writes and what its solvers read
in place of the others -- pinned case by case, without a GPU (the predicates of what the kernels re-derive need the
library only).  Every spectrum path takes its plane set from these functions, so a change here is a change of what the
paths write: tests/golden/plane_choice.json holds what the code they replaced chose (``Spectrum._want_1d`` /
``_want_3d`` and the alias branches of ``Spectrum._plan_1d``) for this file's matrix -- Toon (cloud-free or cloudy; the
legs; Raman off, Pollack, Oklopcic; phase 0, a non-zero phase and phase functions the kernels do not re-derive for; level
fluxes, test mode, all_planes, k-tables, full_output, patchy clouds), SH2 / SH4 (forms, calculate_fluxes, a cloud deck)
and 3-D (clear, cloud tables)."""
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import GOLDEN

NLAYER, NWNO, DECK = 60, 300, 17
CONSTANTS = ("0", "1", "0.5")           # stand-ins for the resident constant planes
THERMAL_READS = {"toon": ("dtau_og", "w0_no_raman", "cosb_og"), "SH": ("dtau", "w0", "cosb_og")}


@pytest.fixture(scope="module")
def lib():
    from picaso_amd import _lib
    from picaso_amd import build as b
    b.build(force=False)              # hipcc cross-compiles; a no-op when the library is current
    return _lib.load()


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(GOLDEN, "plane_choice.json")) as f:
        return json.load(f)


def _inputs(rt="toon", cloud=None, raman="none", phase=0.0, lvl=False, test_mode=None, stream=2, forms=None, fluxes="off",
            holes=False, cloud3=False, approx_kw=None):
    from picaso_amd import justdoit as jdi
    c = jdi.inputs(calculation="planet")
    c.phase_angle(phase, num_gangle=6, num_tangle=6 if phase else 1)
    c.approx(raman=raman, rt_method=rt, stream=stream, get_lvl_flux=lvl, calculate_fluxes=fluxes, **(forms or {}),
             **(approx_kw or {}))
    inp = c.inputs
    inp["test_mode"] = test_mode
    if cloud is not None:             # "all": cloud in every layer; "deck": the top DECK layers clear
        opd, g0 = np.full((NLAYER, 5), 0.1), np.full((NLAYER, 5), 0.5)
        if cloud == "deck":
            opd[:DECK] = g0[:DECK] = 0.0
        inp["clouds"]["profile"] = {"opd": opd, "w0": np.full((NLAYER, 5), 0.9), "g0": g0}
    inp["clouds"]["do_holes"] = holes
    if holes:
        inp["clouds"].update(fhole=0.3, fthin_cld=0.5)
    if cloud3:                        # cloud tables on their own grid (the choice reads only that they exist)
        inp["clouds"]["profile_3d"] = {"opd": np.zeros(3), "w0": np.zeros(3), "g0": np.zeros(3),
                                       "wavenumber": np.arange(3.0)}
    return inp


def _atm(cloud_free=True, lvl=False, rayleigh=True):
    """What the choice reads of an ATMSETUP."""
    return SimpleNamespace(c=SimpleNamespace(nlevel=NLAYER + 1, nlayer=NLAYER), cloud_free=cloud_free,
                           rayleigh_molecules=["H2", "He"] if rayleigh else [], get_lvl_flux=lvl)


def cases_1d():
    """(id, _inputs keywords, _atm keywords, calculation, ngauss, full_output, all_planes)"""
    out = []
    calcs = ("reflected", "thermal", "reflected+thermal", "reflected+thermal+transmission", "transmission")
    for cloud, calc, raman, geo in itertools.product((None, "all"), calcs, ("none", "pollack", "oklopcic"),
                                                     ("phase0", "phase", "otthg")):
        kw = dict(cloud=cloud, raman=raman, phase=0.6 if geo == "phase" else 0.0,
                  approx_kw={"single_phase": "OTHG"} if geo == "otthg" else None)
        out.append(("toon-%s-%s-%s-%s" % (cloud or "clear", calc, raman, geo), kw, dict(cloud_free=cloud is None), calc,
                    1, False, False))
    for cloud, calc in itertools.product((None, "all"), ("reflected", "thermal", "reflected+thermal")):
        tag, akw = cloud or "clear", dict(cloud_free=cloud is None)
        out += [("toon-%s-%s-lvl" % (tag, calc), dict(cloud=cloud, lvl=True), dict(akw, lvl=True), calc, 1, False, False),
                ("toon-%s-%s-testmode" % (tag, calc), dict(cloud=cloud, test_mode="rayleigh"), akw, calc, 1, False, False),
                ("toon-%s-%s-allplanes" % (tag, calc), dict(cloud=cloud), akw, calc, 1, False, True),
                ("toon-%s-%s-ktables" % (tag, calc), dict(cloud=cloud), akw, calc, 3, False, False),
                ("toon-%s-%s-fulloutput" % (tag, calc), dict(cloud=cloud), akw, calc, 1, True, False),
                ("toon-%s-%s-holes" % (tag, calc), dict(cloud=cloud, holes=True), akw, calc, 1, False, False),
                ("toon-%s-%s-norayleigh" % (tag, calc), dict(cloud=cloud), dict(akw, rayleigh=False), calc, 1, False,
                 False)]
    out += [("toon-clear-nolegs-fulloutput", {}, {}, "", 1, True, False),
            ("toon-all-nolegs-fulloutput", dict(cloud="all"), dict(cloud_free=False), "", 1, True, False)]
    forms = {"default": None, "wsingle-othg": {"w_single_form": "OTHG"}, "legendre": {"single_form": "legendre"}}
    for stream, fname, fluxes, cloud, calc in itertools.product(
            (2, 4), forms, ("off", "on"), (None, "all", "deck"), ("reflected", "thermal", "reflected+thermal")):
        out.append(("sh%d-%s-flx%s-%s-%s" % (stream, fname, fluxes, cloud or "clear", calc),
                    dict(rt="SH", stream=stream, forms=forms[fname], fluxes=fluxes, cloud=cloud),
                    dict(cloud_free=cloud is None), calc, 1, False, False))
    for cloud, calc in itertools.product((None, "deck"), ("reflected", "reflected+thermal")):
        for extra, kw, ng, fo, ap in (("allplanes", {}, 1, False, True), ("testmode", {"test_mode": "rayleigh"}, 1, False,
                                                                          False),
                                      ("ktables", {}, 3, False, False), ("fulloutput", {}, 1, True, False),
                                      ("holes", {"holes": True}, 1, False, False)):
            out.append(("sh4-%s-%s-%s" % (cloud or "clear", calc, extra), dict(rt="SH", stream=4, cloud=cloud, **kw),
                        dict(cloud_free=cloud is None), calc, ng, fo, ap))
    return out


def cases_3d():
    """(id, _inputs keywords, calculation, all_planes)"""
    out = []
    for cloud3, calc, raman in itertools.product((False, True), ("reflected", "thermal", "reflected+thermal"),
                                                 ("none", "pollack", "oklopcic")):
        out.append(("3d-%s-%s-%s" % ("cloud" if cloud3 else "clear", calc, raman), dict(cloud3=cloud3, raman=raman),
                    calc, False))
    for cloud3, calc in itertools.product((False, True), ("reflected", "thermal", "reflected+thermal")):
        tag = "cloud" if cloud3 else "clear"
        out += [("3d-%s-%s-testmode" % (tag, calc), dict(cloud3=cloud3, test_mode="rayleigh"), calc, False),
                ("3d-%s-%s-allplanes" % (tag, calc), dict(cloud3=cloud3), calc, True)]
    return out


def _solver_view(legs, refl, rt, calc):
    """What the legs read, by source plane: the aliases among the legs' names, the reflected kernel's own map (None: the
    legs' map) and the three planes of the thermal leg."""
    return {"aliases": {n: v for n, v in sorted(legs.items()) if v != n},
            "refl": None if refl is None else dict(sorted(refl.items())),
            "thermal": [legs[n] for n in THERMAL_READS[rt]] if "thermal" in calc else None}


@pytest.mark.parametrize("case", cases_1d(), ids=lambda c: c[0])
def test_choice_1d(lib, expected, case):
    from picaso_amd import planes
    cid, ikw, akw, calc, ngauss, full_output, all_planes = case
    exp = expected["1d"][cid]
    ch = planes.choose_1d(_inputs(**ikw), _atm(**akw), NWNO, ngauss, calc, full_output, all_planes)
    assert (None if ch.want is None else sorted(ch.want)) == exp["want"]
    assert (ch.lean, ch.derive, ch.sh_lean, ch.sh_top) == (exp["lean"], exp["derive"], exp["sh_lean"], exp["sh_top"])
    legs, refl = planes.views(ch, {k: k for k in (planes.OUT_NAMES if ch.want is None else ch.want)}, lambda: CONSTANTS)
    rt = ikw.get("rt", "toon")
    assert _solver_view(legs, None if refl is legs else refl, rt, calc) == exp["view"]
    if "thermal" in calc:             # the driver hands the thermal kernels the planes the Choice names
        assert ch.thermal == THERMAL_READS[rt]
    else:
        assert ch.thermal is None


@pytest.mark.parametrize("case", cases_3d(), ids=lambda c: c[0])
def test_choice_3d(lib, expected, case):
    from picaso_amd import planes
    cid, ikw, calc, all_planes = case
    exp = expected["3d"][cid]
    ch = planes.choose_3d(_inputs(**ikw), calc, all_planes)
    assert sorted(ch.want) == exp["want"]
    assert (None if ch.thermal is None else list(ch.thermal)) == exp["th3"]
    assert not (ch.lean or ch.derive or ch.sh_lean or ch.sh_top)


def test_matrix_covers_every_pinned_case(expected):
    assert sorted(c[0] for c in cases_1d()) == sorted(expected["1d"])
    assert sorted(c[0] for c in cases_3d()) == sorted(expected["3d"])


def test_cloud_free_top_is_reexported():
    from picaso_amd import justdoit as jdi
    from picaso_amd import planes
    assert jdi._cloud_free_top is planes.cloud_free_top
    assert planes.cloud_free_top(_inputs(cloud="deck"), NLAYER) == DECK
    assert planes.cloud_free_top(_inputs(), NLAYER) == NLAYER
