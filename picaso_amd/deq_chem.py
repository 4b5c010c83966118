"""On-the-fly correlated-k gas mixing with the reference's call signature.

Drop-in for ``picaso.deq_chem.mix_all_gases_gasesfly`` (reference picaso/deq_chem.py:333-384): numpy
arrays in, the ``(nlayer, nwno, ngauss, 4)`` array of ln(mixed k) out.  The per-gas tables are large
(tens of MB each) and do not change between calls of a climate run, so their device copies are kept
and reused for host arrays with the same content (keyed by a digest of every byte, not by address).
``picaso_amd.optics.RetrieveCKs(kappas=...)`` is the resident form ``picaso()`` uses.

``get_quench_levels`` / ``OH_conc`` (reference deq_chem.py:5-150) are the quench approximation of the climate solve: host
code on one profile of ~100 levels.
"""
import os

import numpy as np

from . import _lib, resident
from ._lib import f64
from .device import DeviceArray

_tables = {}            # (pid, context, digest of the table) -> DeviceArray: content-addressed, oldest out first
_TABLES_MAX = 64
_lib.on_context_destroy(lambda value: [_tables.pop(k) for k in [k for k in _tables if k[1] == value]])


def _fingerprint(a):
    """Digest of every byte of the table (``optics.content_digest``): an in-place edit of one coefficient is a new
    table, as it is for the reference, which reads its arguments afresh on every call (deq_chem.py:334-384)."""
    from .optics import content_digest
    return content_digest(a)


def _resident_table(a, ctx):
    a = f64(a)
    key = (os.getpid(), getattr(ctx, "value", ctx), _fingerprint(a))
    hit = _tables.get(key)
    if hit is not None:
        return hit
    while len(_tables) >= _TABLES_MAX:
        del _tables[next(iter(_tables))]
    d = DeviceArray.from_host(a, ctx)
    _tables[key] = d
    return d


def clear_table_cache():
    """Drop the device copies of the k-tables kept by ``mix_all_gases_gasesfly``."""
    _tables.clear()


@_lib.serialized
def mix_all_gases_gasesfly(kappas, mixes, gauss_pts, gauss_wts, indices, ctx=None):
    """``kappas``: list of ``(npres, ntemp, nwno, ngauss)`` ln(kappa) arrays, ``mixes``: list of per-layer
    mixing ratios, ``indices`` = [p_low, p_hi, t_low, t_hi] per layer (``get_mixing_indices``).
    Returns ``(nlayer, nwno, ngauss, 4)``: ln of the mixed coefficients at the four P-T neighbours."""
    ctx = ctx if ctx is not None else _lib.context()
    dk = [_resident_table(k, ctx) for k in kappas]
    out = resident.mix_all_gases_gasesfly(ctx, dk, mixes, gauss_pts, gauss_wts, indices).to_host()
    return np.ascontiguousarray(np.moveaxis(out, 1, 3))


def OH_conc(temp, press, x_h2o, x_h2):
    """Number density of OH (cm^-3) in equilibrium with H2O and H2 at ``temp`` (K) and ``press`` (bar), from volume mixing
    ratios (reference deq_chem.py:141-150)."""
    K = 10 ** (3.672 - (14791 / temp))
    x_oh = K * x_h2o * (x_h2 ** (-0.5)) * (press ** (-0.5))
    n = press * 1e6 / (1.3807e-16 * temp)
    return x_oh * n


def _pad(a, n):
    a = np.asarray(a, dtype=float)
    return a if len(a) >= n else np.append(a, np.full(n - len(a), a[-1]))


def get_quench_levels(Atmosphere, kz, grav, mh_linear, PH3=True, H2O=None, H2=None):
    """Quench levels of the Zahnle & Marley (2014) time scales against the mixing time ``t_mix = H^2 / kz`` (reference
    deq_chem.py:5-139).  ``Atmosphere``: ``t_level, p_level`` (bar), ``dtdp, mmw_layer, scale_height``; ``kz`` in cm^2/s;
    ``grav`` in m/s^2 (what the climate driver carries: the constant-gravity scale height is then in cm);
    ``mh_linear``: metallicity, 3 for 3 x solar.  Returns ``({name: level}, t_mix)`` with names ``CO-CH4-H2O`` (time scale
    ``mh_linear**-0.7``), ``CO2``, ``NH3-N2``, ``HCN`` (``mh_linear**0.7``) and, with ``PH3``, ``PH3`` (through ``OH_conc`` of
    the ``H2O`` and ``H2`` mixing ratios).

    Kept from the reference:
    * a gas quenches at the first level pair from the bottom up with ``t_mix[j-1] <= t_chem[j-1]`` and ``t_mix[j] >=
      t_chem[j]``; the stored level is ``min(j, nlevel - 2)``; without such a pair the name is absent;
    * ``max(t_mix) < min(t_chem)`` raises (the reference's messages), for every gas but PH3;
    * the constant-gravity scale height is overwritten by ``Atmosphere.scale_height`` where that exists; ``mmw``, ``kz``,
      ``H2O`` and ``H2`` are padded with their last value;
    * a cold profile (``min(T) <= 250``) whose deepest pressure is below 1e6 bar is continued by ten levels,
      ``logspace(log10(p[-1] + 100), 6, 10)``, with the lapse rate ``dtdp[-1]``: a level may then be ``>= `` the length of the
      profile handed in (``inputs.adjust_quench_chemistry`` extends the chemistry the same way)."""
    temp, pressure = np.asarray(Atmosphere.t_level, dtype=float), np.asarray(Atmosphere.p_level, dtype=float)
    dtdp, scale_height = Atmosphere.dtdp, Atmosphere.scale_height
    k_b, m_p = 1.38e-23, 1.66e-27
    nlevel = len(temp)
    if np.min(temp) <= 250 and pressure[-1] < 1e6:
        pressure = np.append(pressure, np.logspace(np.log10(pressure[-1] + 100), 6, 10))
        for i in range(nlevel, nlevel + 10):
            temp = np.append(temp, np.exp(np.log(temp[i - 1]) - dtdp[-1] * (np.log(pressure[i - 1]) - np.log(pressure[i]))))
        nlevel = len(temp)
    mmw = _pad(Atmosphere.mmw_layer, nlevel)
    scale_H = k_b / (mmw * m_p) * temp * 1e2 / grav
    if scale_height is not None:
        scale_H[0:len(scale_height)] = scale_height
    kz = _pad(kz, nlevel)
    t_mix = scale_H ** 2 / kz

    quench_levels = {}

    def scan(name, t_chem, what):
        if what is not None and np.max(t_mix) < np.min(t_chem):
            raise Exception("%s mixing across Pressure Ranges, Start with deeper Pressure Grid" % what)
        for j in range(nlevel - 1, 0, -1):
            if (t_mix[j - 1] / 1e15 <= t_chem[j - 1] / 1e15) and (t_mix[j] / 1e15 >= t_chem[j] / 1e15):
                quench_levels[name] = min(j, nlevel - 2)
                break
    scan("CO-CH4-H2O", (1.5e-6 / pressure * mh_linear ** -0.7) * np.exp(42000 / temp), "CO/H2O/CH4")
    scan("CO2", (1e-10 / (pressure ** 0.5)) * np.exp(38000. / temp), "CO2")
    scan("NH3-N2", (1e-7 / pressure) * np.exp(52000 / temp), "NH3")
    scan("HCN", (1.5e-4 / (pressure * (mh_linear ** 0.7))) * np.exp(36000. / temp), "HCN")
    if PH3:
        OH = OH_conc(temp, pressure, _pad(H2O, nlevel), _pad(H2, nlevel))
        scan("PH3", 0.19047619047 * 1e13 * np.exp(6013.6 / temp) / OH, None)
    return quench_levels, t_mix
