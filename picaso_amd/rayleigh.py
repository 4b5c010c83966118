"""Rayleigh scattering cross sections per species on a wavenumber grid (counterpart of the reference
``picaso/rayleigh.py``): host-side numpy, evaluated once per opacity object -- the reference does the same when an
opacity object is opened (``get_available_rayleigh``, optics.py:1060-1065, :2041-2046).  No database carries them.

    sigma(nu) = 24 pi^3 nu^4 / n_ref^2 * ((eta^2 - 1) / (eta^2 + 2))^2 * F_King * N_A

with the refractive index ``eta`` at the reference number density ``n_ref`` (0 C, 1 atm) from, in this order,

* a dispersion fit of its own for the species of ``_HOHM`` (two-oscillator polarisability, Hohm 1993) and of ``_FITS``
  (piecewise refractivity fits in wavelength, constant outside their range),
* the Lorentz-Lorenz relation on a constant polarisability (``POLARISABILITIES``, mostly the CRC handbook),
* ``eta = 0`` for a name in neither table, which is what the reference computes for it (a cross section of
  6 pi^3 nu^4 / n_ref^2 * N_A; such a name is not in ``rayleigh_molecules`` and no opacity object asks for it).

The King correction is wavelength dependent where the fit gives it, a constant from ``KING_CORRECTION`` (Bogaard+ 1978;
O3: Brasseur & De Rudder 1986), else 1.  The constants below are the published values the reference restates.
"""
import numpy as np

BOLTZMANN = 1.380649e-23            # J/K (SI 2019, exact)
AVOGADRO = 6.02214086e+23           # the value of the opacity sums (optics.AVOGADRO)
N_REF = (101325.0 / (BOLTZMANN * 273.15)) * 1.0e-6          # cm^-3 at 0 C, 1 atm
HARTREE_WNO = 219474.6305           # cm^-1 per atomic unit of energy
BOHR3_CM3 = 0.148184e-24            # cm^3 per atomic unit of polarisability
T15_OVER_T0 = 288.15 / 273.15       # refractivities measured at 15 C, scaled to 0 C (Sneep & Ubachs 2005)

POLARISABILITIES = {                # cm^3
    "H2": 0.80e-24, "He": 0.21e-24, "N2": 1.74e-24, "O2": 1.58e-24, "O3": 3.21e-24, "H2O": 1.45e-24, "CH4": 2.59e-24,
    "CO": 1.95e-24, "CO2": 2.91e-24, "NH3": 2.26e-24, "HCN": 2.59e-24, "PH3": 4.84e-24, "SO2": 3.72e-24, "SO3": 4.84e-24,
    "C2H2": 3.33e-24, "H2S": 3.78e-24, "NO": 1.70e-24, "NO2": 3.02e-24, "H3+": 0.385e-24, "OH": 6.965e-24,
    "Na": 24.11e-24, "K": 42.9e-24, "Li": 24.33e-24, "Rb": 47.39e-24, "Cs": 59.42e-24, "TiO": 16.9e-24, "VO": 14.4e-24,
    "AlO": 8.22e-24, "SiO": 5.53e-24, "CaO": 23.8e-24, "TiH": 16.9e-24, "MgH": 10.5e-24, "NaH": 24.11e-24, "AlH": 8.22e-24,
    "CrH": 11.6e-24, "FeH": 9.47e-24, "CaH": 23.8e-24, "BeH": 5.60e-24, "ScH": 21.2e-24}

KING_CORRECTION = {"O3": 1.060000, "CO": 1.016995, "C2H2": 1.064385, "C2H6": 1.006063, "OCS": 1.138786,
                   "CH3Cl": 1.026042, "H2S": 1.001880, "SO2": 1.062638}

# Two-oscillator fits of the polarisability parallel and perpendicular to the axis (Hohm 1993), atomic units:
# (f_par, w_par^2, f_perp, w_perp^2).  Mean polarisability (a_par + 2 a_perp) / 3, anisotropy a_par - a_perp.
_HOHM = {
    "CO2": (6.00332, 0.22525399, 8.54433, 0.66083749),
    "H2": (1.62632, 0.23940245, 1.40105, 0.29486069),
    "N2O": (5.65126, 0.17424213, 9.72095, 0.72904985),
    "NH3": (1.28964, 0.08454599, 10.84943, 0.76338846),
    "O2": (2.74876, 0.18095751, 4.86007, 0.58545449)}

# Piecewise refractive-index fits.  ``edges``: wavelengths (micron) between the pieces -- below the first edge (strictly)
# the first piece holds, an edge itself belongs to the piece below it otherwise.  A piece is a constant ``eta`` (a float)
# or a list of refractivity terms summed to ``eta - 1``:
#   ("const", c)          c
#   ("nu2", c)            c * nu^2                          nu in cm^-1
#   ("pole_nu2", a, b)    a / (b - nu^2)
#   ("pole_um", a, b)     a / (b - 1 / lambda^2)            lambda in micron
#   ("hill_lawrence", ..) the second term of the water-vapour fit of Hill & Lawrence 1986
# times ``scale`` (a continuity factor between two fits).  ``t15``: the whole fit is for 15 C.  ``king``: (k0, k2) of
# F = k0 + k2 nu^2.
_FITS = {
    "CH4": dict(edges=(0.325, 0.633), t15=True, king=(1.0, 0.0), pieces=(             # Sneep & Ubachs 2005, Hohm 1993
        1.000504679, (1.0, [("const", 46662.0e-8), ("nu2", 4.02e-14)]), 1.000476653)),
    "H2O": dict(edges=(0.360, 17.60), t15=False, king=(1.001005, 0.0), pieces=(       # Hill & Lawrence 1986; n >= 1
        1.000258047,
        (1.0, [("pole_um", 3.011e-2, 124.40), ("hill_lawrence", 7.46e-3, 0.203, 1.03, 1.98e3, 8.1e4, 1.7e8)]),
        1.000000000)),
    "He": dict(edges=(0.2753, 0.4801, 2.0586), t15=False, king=(1.0, 0.0), pieces=(   # Cuthbertson 1936; Mansfield & Peck 1969
        1.00003578, (1.0018141444038913, [("pole_um", 0.014755297, 426.29740)]),
        (1.0, [("pole_um", 0.01470091, 423.98)]), 1.00003469)),
    "N2": dict(edges=(0.2540, 0.46816, 2.0576), t15=True, king=(1.034, 3.17e-12), pieces=(   # Bates 1984; Peck & Khanna 1966
        1.00030493, (1.0001468057477378, [("const", 5677.465e-8), ("pole_nu2", 318.81874e4, 14.4e9)]),
        (1.0, [("const", 6498.2e-8), ("pole_nu2", 307.43305e4, 14.4e9)]), 1.00027883))}


def _lorentz_lorenz(alpha):
    """Refractive index of a gas of polarisability ``alpha`` (cm^3) at the number density N_REF."""
    x = 4.0 * np.pi * N_REF * alpha / 3.0
    return np.sqrt((1.0 + 2.0 * x) / (1.0 - x))


def _term(term, nu, wl):
    kind = term[0]
    if kind == "const":
        return np.full(nu.shape, term[1])
    if kind == "nu2":
        return term[1] * nu ** 2
    if kind == "pole_nu2":
        return term[1] / (term[2] - nu ** 2)
    if kind == "pole_um":
        return term[1] / (term[2] - 1.0 / wl ** 2)
    if kind == "hill_lawrence":
        _, a, b, c0, c2, c4, c8 = term
        return (a * (b - 1.0 / wl)) / (c0 - c2 / wl ** 2 + c4 / wl ** 4 - c8 / wl ** 8)
    raise KeyError(kind)


def refractive_index(species, nu):
    """``(eta, F)``: refractive index at N_REF and King correction factor of ``species`` on the wavenumbers ``nu``."""
    nu = np.asarray(nu, dtype=np.float64)
    one = np.ones(nu.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        wl = 1e4 / nu
        if species in _HOHM:
            f_par, w_par, f_perp, w_perp = _HOHM[species]
            e2 = (nu / HARTREE_WNO) ** 2
            a_par, a_perp = f_par / (w_par - e2), f_perp / (w_perp - e2)
            alpha = (1.0 / 3.0) * (a_par + 2.0 * a_perp)
            eta = _lorentz_lorenz(alpha * BOHR3_CM3)
            return eta, 1.0 + 2.0 * ((a_par - a_perp) / (3.0 * alpha)) ** 2
        if species in _FITS:
            fit = _FITS[species]
            edges = fit["edges"]
            piece = (wl >= edges[0]).astype(np.intp)
            for e in edges[1:]:
                piece += wl > e
            eta = np.empty(nu.shape)
            for i, p in enumerate(fit["pieces"]):
                sel = piece == i
                if isinstance(p, float):
                    eta[sel] = p
                elif sel.any():
                    scale, terms = p
                    eta[sel] = 1.0 + sum(_term(t, nu[sel], wl[sel]) for t in terms) * scale
            if fit["t15"]:
                eta = (eta - 1.0) * T15_OVER_T0 + 1.0
            k0, k2 = fit["king"]
            return eta, (k0 + k2 * nu ** 2 if k2 else k0 * one)
        eta = _lorentz_lorenz(POLARISABILITIES[species] * one) if species in POLARISABILITIES else 0.0 * nu
        return eta, KING_CORRECTION.get(species, 1.0) * one


class Rayleigh:
    """The reference class's surface: ``Rayleigh(wavenumber).compute_sigma(species)``.

    Attributes: ``wno`` (cm^-1), ``wavelength`` (micron), ``n_ref`` (cm^-3 at 0 C and 1 atm), ``polarisabilities`` (cm^3),
    ``king_correction_no_wave``, ``rayleigh_molecules`` (the keys of ``polarisabilities``: the species an opacity
    object computes)."""

    def __init__(self, wavenumber):
        self.wno = wavenumber
        with np.errstate(divide="ignore"):
            self.wavelength = 1e4 / wavenumber
        self.n_ref = N_REF
        self.polarisabilities = dict(POLARISABILITIES)
        self.king_correction_no_wave = dict(KING_CORRECTION)
        self.rayleigh_molecules = list(POLARISABILITIES.keys())

    def refractive_index(self, species):
        """``(eta, F)`` of ``species`` (case-sensitive: TiH, not TIH) on the grid."""
        return refractive_index(species, self.wno)

    def compute_sigma(self, species):
        """Rayleigh cross section of ``species`` times Avogadro's number, (nwno,), the reference's units: the opacity
        sums multiply it by column density * mixing ratio / mean molecular weight (optics.py:265-271)."""
        nu = np.asarray(self.wno, dtype=np.float64)
        eta, king = refractive_index(species, nu)
        lorentz = (eta ** 2 - 1.0) / (eta ** 2 + 2.0)
        return ((24.0 * np.pi ** 3 * nu ** 4) / N_REF ** 2) * lorentz ** 2 * king * AVOGADRO


def available_rayleigh(wno):
    """``{species: sigma(wno)}`` for every species of ``rayleigh_molecules``, in that order: what an opacity object
    holds when the caller supplies no cross sections (reference ``get_available_rayleigh``)."""
    ray = Rayleigh(np.asarray(wno, dtype=np.float64))
    return {m: ray.compute_sigma(m) for m in ray.rayleigh_molecules}
