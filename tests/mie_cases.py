"""What tests/test_mie_host.py and tests/test_mie_gpu.py share: the fixed list of Mie cases, the series of picaso_amd/mie.py
restated in 40-digit mpmath (the arbiter), the three error measures, and a small synthetic Mie table."""
import functools

import numpy as np

U = 2.0 ** -53


def case_list():
    """64 cases: 61 seeded ones -- x log-uniform in [1e-6, 1e3], n in [1.05, 3], k = 0 for every tenth and otherwise
    log-uniform in [1e-8, 3] -- and x = 3000 with a weakly, a moderately and a strongly absorbing index."""
    rng = np.random.default_rng(20261021)
    count = 61
    x = 10 ** rng.uniform(-6, 3, count)
    n = rng.uniform(1.05, 3, count)
    k = 10 ** rng.uniform(-8, np.log10(3), count)
    k[::10] = 0
    return np.r_[x, 3000.0, 3000.0, 3000.0], np.r_[n + 1j * k, 1.33 + 1e-8j, 1.5 + 0.01j, 1.7 + 0.3j]


def mie_mpmath(x, m, dps=40):
    """``(qext, qsca, g qsca)`` of one sphere as mpmath numbers: the formulae of picaso_amd/mie.py on the exact values of the
    doubles ``x`` and ``m``, with the downward recurrences started ``30 |y|^(1/3)`` higher."""
    import mpmath as mp
    with mp.workdps(dps):
        x = mp.mpf(float(x))
        m = mp.mpc(float(np.real(m)), float(np.imag(m)))
        y = m * x
        ay = abs(y)
        nstop = int(x + 4 * mp.cbrt(x) + 2)
        nmx = int(max(nstop, ay) + 15 + 8 * mp.cbrt(ay) + 30 * mp.cbrt(ay))
        dy, dx = [mp.mpc(0)] * (nmx + 1), [mp.mpf(0)] * (nmx + 1)
        for n in range(nmx, 0, -1):
            dy[n - 1] = n / y - 1 / (dy[n] + n / y)
            dx[n - 1] = n / x - 1 / (dx[n] + n / x)
        psi1, chi1, chi2 = mp.sin(x), mp.cos(x), -mp.sin(x)
        a1 = b1 = mp.mpc(0)
        qext = qsca = gqsc = mp.mpf(0)
        for n in range(1, nstop + 1):
            psi = psi1 / (dx[n] + n / x)
            chi = (2 * n - 1) / x * chi1 - chi2
            xi, xi1 = mp.mpc(psi, -chi), mp.mpc(psi1, -chi1)
            ca, cb = dy[n] / m + n / x, m * dy[n] + n / x
            an = (ca * psi - psi1) / (ca * xi - xi1)
            bn = (cb * psi - psi1) / (cb * xi - xi1)
            qext += (2 * n + 1) * (an + bn).real
            qsca += (2 * n + 1) * (abs(an) ** 2 + abs(bn) ** 2)
            gqsc += (mp.mpf(2 * n + 1) / (n * (n + 1)) * (an * mp.conj(bn)).real
                     + mp.mpf((n - 1) * (n + 1)) / n * (a1 * mp.conj(an) + b1 * mp.conj(bn)).real)
            psi1, chi2, chi1, a1, b1 = psi, chi1, chi, an, bn
        return 2 / x ** 2 * qext, 2 / x ** 2 * qsca, 4 / x ** 2 * gqsc


@functools.lru_cache(maxsize=None)
def reference():
    """The mpmath values of every case of ``case_list``, computed once per process."""
    x, m = case_list()
    return tuple(mie_mpmath(xi, mi) for xi, mi in zip(x, m))


def errors(q):
    """``(3, ncase)`` errors of ``q = (qext, qsca, g qsca)`` arrays against ``reference()``: relative in Qext, relative in
    Qsca, and |delta| / Qsca in g Qsca (the absolute error of g: g Qsca itself vanishes like x^6)."""
    import mpmath as mp
    out = np.empty((3, len(reference())))
    with mp.workdps(40):
        for i, (e, s, g) in enumerate(reference()):
            out[0, i] = float(abs(mp.mpf(float(q[0][i])) - e) / e)
            out[1, i] = float(abs(mp.mpf(float(q[1][i])) - s) / s)
            out[2, i] = float(abs(mp.mpf(float(q[2][i])) - g) / s)
    return out


def synthetic_table(nwave=7, nradii=4, seed=3, lo_um=0.4, hi_um=12.0, increasing=False):
    """A smooth positive Mie-like table (no Mie series behind it): ``qext > qscat > |cos_qscat|``.  Rows arrive wavelength
    decreasing (wavenumber increasing) unless ``increasing``."""
    from picaso_amd import mie
    rng = np.random.default_rng(seed)
    wave = np.geomspace(hi_um, lo_um, nwave)
    radius = np.geomspace(1e-5, 3e-3, nradii) if nradii > 1 else np.array([2e-4])
    xs = 2 * np.pi * radius[None, :] * 1e4 / wave[:, None]
    qext = 2.0 * xs ** 2 / (1.0 + xs ** 2) + 0.05 + 0.01 * rng.random(xs.shape)
    qscat = qext * (0.3 + 0.6 / (1.0 + 0.1 * xs)) * (1.0 - 0.01 * rng.random(xs.shape))
    cos_qscat = qscat * (0.8 * xs / (1.0 + xs) - 0.05)
    if increasing:
        qext, qscat, cos_qscat, wave = qext[::-1], qscat[::-1], cos_qscat[::-1], wave[::-1]
    return mie.MieTable(qext, qscat, cos_qscat, radius, wave)
