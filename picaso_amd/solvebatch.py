"""The Toon solver launches of a spectrum as records: launched at once, or collected and launched together.

``Spectrum`` describes each monochromatic Toon solve as a ``Solve`` -- its leg, its context, a named grouping key (shape
and options: what a launch is compiled and configured for) and its own arguments -- and either launches it alone
(``launch``) or hands it to a ``SolveBatch`` (``spectrum_batch`` / ``phase_curve``), whose ``flush()`` issues ONE batched
launch per group of records with equal keys (``picaso_get_*_batch_dev``): every spectrum is bit-identical to its own
launch, the GPU sees one grid that fills it instead of B that each leave its SIMDs half empty (DESIGN.md sections 5 and 6).
Each leg is described once, in ``LEGS``: how one record goes alone, how a group goes together, and whether it may.
"""
from collections import namedtuple

import numpy as np

from . import resident

# grouping keys.  ``present`` (the planes handed over) and ``wno`` (the address of the resident wavenumber grid) are not
# arguments of a launch: they keep records apart that cannot share one.
Reflected1D = namedtuple("Reflected1D", "nlevel nwno numg numt tthg toon_coefficients b_top gweight tweight present")
Thermal1D = namedtuple("Thermal1D", "nlevel nwno numg numt hard_surface wno gweight tweight")
Reflected3D = namedtuple("Reflected3D", "nlevel nwno numg numt tthg present facet_major gweight tweight")
Thermal3D = namedtuple("Thermal3D", "nlevel nwno numg numt hard_surface wno has_cosb facet_major gweight tweight")

# one pending solve.  ``args``: the per-spectrum arguments by name; ``keep`` holds planes alive until the launch.
Solve = namedtuple("Solve", "leg ctx key args keep", defaults=(None,))


def _column(group, name):
    return [r.args[name] for r in group]


def _stacked(group, name):
    """A geometry argument of every member: ``(nspec, numg, numt)``, or ``(nspec,)`` for ``cos_theta``."""
    k = group[0].key
    if name == "cos_theta":
        return np.array(_column(group, name), dtype=float)
    return np.stack([np.asarray(a, dtype=float).reshape(k.numg, k.numt) for a in _column(group, name)])


def _shared_or_stacked(group, names):
    """Equal geometry across a 1-D group collapses to the single-geometry call."""
    first = group[0].args
    if all(np.array_equal(r.args[n], first[n]) for r in group for n in names):
        return [first[n] for n in names]
    return [_stacked(group, n) for n in names]


def _small_disk_group(group):
    """The batched 1-D launches carry at most 8 disk angles (a 6 x 6 disk goes alone), and one member needs none."""
    return len(group) > 1 and group[0].key.numg * group[0].key.numt <= 8


def _reflected_1d(r):
    k, a = r.key, r.args
    resident.reflected_1d(r.ctx, k.nlevel, k.nwno, k.numg, k.numt, a["planes"], a["rs"], a["ubar0"], a["ubar1"],
                          a["cos_theta"], a["F0PI"], *k.tthg, a["xint"], toon_coefficients=k.toon_coefficients,
                          b_top=k.b_top, gweight=k.gweight, tweight=k.tweight, albedo=a["albedo"], lvl_fluxes=a.get("lvl"))


def _reflected_1d_group(group):
    k = group[0].key
    u0, u1, ct = _shared_or_stacked(group, ("ubar0", "ubar1", "cos_theta"))
    resident.reflected_1d_batch(group[0].ctx, k.nlevel, k.nwno, k.numg, k.numt, _column(group, "planes"),
                                _column(group, "rs"), u0, u1, ct, _column(group, "F0PI"), *k.tthg, _column(group, "xint"),
                                toon_coefficients=k.toon_coefficients, b_top=k.b_top, gweight=k.gweight, tweight=k.tweight,
                                albedo=_column(group, "albedo"))


def _thermal_1d(r):
    k, a = r.key, r.args
    fused = dict(gweight=k.gweight, tweight=k.tweight, flux_disk=a["disk"]) if a["disk"] is not None else {}
    resident.thermal_1d(r.ctx, k.nlevel, a["wno"], k.nwno, k.numg, k.numt, a["tlevel"], a["dtau"], a["w0"], a["cosb"],
                        a["plevel"], a["ubar1"], a["rs"], k.hard_surface, a["flux"], lvl_fluxes=a.get("lvl"), **fused,
                        **a.get("options", {}))


def _thermal_1d_group(group):
    k = group[0].key
    u1, = _shared_or_stacked(group, ("ubar1",))
    resident.thermal_1d_batch(group[0].ctx, k.nlevel, group[0].args["wno"], k.nwno, k.numg, k.numt,
                              np.stack(_column(group, "tlevel")), _column(group, "dtau"), _column(group, "w0"),
                              _column(group, "cosb"), np.stack(_column(group, "plevel")), u1, _column(group, "rs"),
                              k.hard_surface, _column(group, "flux"), gweight=k.gweight, tweight=k.tweight,
                              flux_disk=_column(group, "disk"))


def _reflected_3d(r):
    k, a = r.key, r.args
    if k.facet_major:                                # one spectrum through the facet-major batch: each facet a spectrum
        return _reflected_3d_group([r])
    resident.reflected_3d(r.ctx, k.nlevel, k.nwno, k.numg, k.numt, a["planes"], a["rs"], a["ubar0"], a["ubar1"],
                          a["cos_theta"], a["F0PI"], *k.tthg, a["xint"], k.gweight, k.tweight, a["albedo"])


def _reflected_3d_group(group):
    k = group[0].key
    fn = resident.reflected_3d_fm_batch if k.facet_major else resident.reflected_3d_batch
    fn(group[0].ctx, k.nlevel, k.nwno, k.numg, k.numt, _column(group, "planes"), _column(group, "rs"),
       _stacked(group, "ubar0"), _stacked(group, "ubar1"), _stacked(group, "cos_theta"), _column(group, "F0PI"), *k.tthg,
       _column(group, "xint"), gweight=k.gweight, tweight=k.tweight, albedo=_column(group, "albedo"))


def _thermal_3d(r):
    k, a = r.key, r.args
    if k.facet_major:
        return _thermal_3d_group([r])
    resident.thermal_3d(r.ctx, k.nlevel, a["wno"], k.nwno, k.numg, k.numt, a["tlevel"], a["dtau"], a["w0"], a["cosb"],
                        a["plevel"], a["ubar1"], a["rs"], k.hard_surface, a["flux"], k.gweight, k.tweight, a["disk"])


def _thermal_3d_group(group):
    k = group[0].key
    fn = resident.thermal_3d_fm_batch if k.facet_major else resident.thermal_3d_batch
    fn(group[0].ctx, k.nlevel, group[0].args["wno"], k.nwno, k.numg, k.numt, np.stack(_column(group, "tlevel")),
       _column(group, "dtau"), _column(group, "w0"), _column(group, "cosb") if k.has_cosb else None,
       np.stack(_column(group, "plevel")), _stacked(group, "ubar1"), _column(group, "rs"), k.hard_surface,
       _column(group, "flux"), gweight=k.gweight, tweight=k.tweight, flux_disk=_column(group, "disk"))


# leg -> (one record alone, a group together, may this group go together), in the order ``flush()`` launches them.
# 3-D groups always use the batch entry, also for a single member.
Leg = namedtuple("Leg", "alone together may_batch")
LEGS = {
    "reflected_3d": Leg(_reflected_3d, _reflected_3d_group, lambda group: True),
    "thermal_3d": Leg(_thermal_3d, _thermal_3d_group, lambda group: True),
    "reflected_1d": Leg(_reflected_1d, _reflected_1d_group, _small_disk_group),
    "thermal_1d": Leg(_thermal_1d, _thermal_1d_group, _small_disk_group),
}


def launch(solve):
    """The record's own launch, now."""
    LEGS[solve.leg].alone(solve)


class SolveBatch:
    """The pending solves of several ``picaso(defer=True, _batch=...)`` calls, grouped by leg and key in the order they
    were added; ``flush()`` launches them."""

    def __init__(self):
        self.groups = {leg: {} for leg in LEGS}

    def add(self, solve):
        self.groups[solve.leg].setdefault(solve.key, []).append(solve)

    def pending(self):
        return sum(len(group) for groups in self.groups.values() for group in groups.values())

    def flush(self):
        for name, leg in LEGS.items():
            for group in self.groups[name].values():
                if leg.may_batch(group):
                    leg.together(group)
                else:
                    for solve in group:
                        leg.alone(solve)
            self.groups[name] = {}
