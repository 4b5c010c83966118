"""Mie clouds: Mie efficiencies made on the GPU, the table and file they live in, the sum of a table over a particle-size
distribution, the reference's two size-dependent cloud forms, and their batch in HBM.

The reference borrows three things from virga for ``Parameterize.cloud_brewster_mie`` and ``cloud_flex_fsed`` (reference
picaso/parameterizations.py:29-32, 59-80, 94-198): a table of Mie efficiencies per (wavelength, radius), a reader for it
(``vj.get_mie``) and one sum of it over a size distribution (``vj.calc_optics_user_r_dist``).  This module builds the three
here, so that neither virga nor its files are needed.  The methods of ``Parameterize`` with those names keep refusing
(tests pin their words); the functions of this module take a ``Parameterize`` and do the job.

The Mie series (``mie_efficiencies`` on the device, csrc/mie.hip; ``mie_efficiencies_numpy`` the same arithmetic on the
host).  For a size parameter ``x = 2 pi r / lambda`` and a refractive index ``m = n + ik`` (``k >= 0``), with ``y = m x``:

    nstop = int(x + 4 x^(1/3) + 2)
    nmx   = int(max(nstop, |y|) + 15 + 8 |y|^(1/3))
    D_nmx(y) = 0,  D_{n-1}(y) = n/y - 1/(D_n(y) + n/y)         downward, complex
    D_nmx(x) = 0,  D_{n-1}(x) = n/x - 1/(D_n(x) + n/x)         downward, real
    psi_0 = sin x,               psi_n = psi_{n-1} / (D_n(x) + n/x)              the ratio form, upward
    chi_0 = cos x, chi_-1 = -sin x,  chi_n = (2n-1)/x chi_{n-1} - chi_{n-2}      upward
    xi_n = psi_n - i chi_n
    a_n = ((D_n(y)/m + n/x) psi_n - psi_{n-1}) / ((D_n(y)/m + n/x) xi_n - xi_{n-1})
    b_n = ((m D_n(y) + n/x) psi_n - psi_{n-1}) / ((m D_n(y) + n/x) xi_n - xi_{n-1})
    Qext  = 2/x^2 sum (2n+1) Re(a_n + b_n)
    Qsca  = 2/x^2 sum (2n+1) (|a_n|^2 + |b_n|^2)
    gQsca = 4/x^2 sum [ (2n+1)/(n(n+1)) Re(a_n conj b_n) + (n-1)(n+1)/n Re(a_{n-1} conj a_n + b_{n-1} conj b_n) ]

every sum over n = 1 .. nstop in increasing n.  ``gQsca`` is what virga's files call ``cos_qscat``.  Two things differ from
the textbook (Bohren & Huffman's BHMIE): the ``8 |y|^(1/3)`` in ``nmx``, without which the downward recurrence of a weakly
absorbing large sphere has not converged when it reaches ``nstop`` (up to 3e-3 in Qext), and the ratio form of ``psi``,
without which the upward three-term recurrence loses Qext for small ``x``.  Against 50-60 digit mpmath the algorithm as
stated stays within 6.3e-14 (relative in Qext and Qsca, absolute in g) for 1e-6 <= x <= 3200.

``x <= 0``, a NaN anywhere or ``k < 0`` gives NaN in that element.  An ``nmx`` above ``NMX_CAP`` is an error.
"""
import os

import numpy as np

NMX_CAP = 1 << 20                   # most terms of one series (csrc/mie.hip: MIE_NMX_CAP), x of about 1e6
SCRATCH_BYTES = 256 << 20           # device scratch of one launch of mie_efficiencies: longer lists run in chunks
_WAVE = 64                          # lanes of a wave: the unit the scratch is laid out for
PI = np.pi

LAUNCHES = 0                        # cloud-table launches of this process so far
MIE_LAUNCHES = 0                    # launches (chunks) of mie_efficiencies of this process so far
TABLE_UPLOADS = 0                   # MieTables uploaded by this process so far (a memo hit does not count)


# ---------------------------------------------------------------------------------------------------- the Mie series
def _orders(x, m):
    """``(valid, nstop, nmx)`` of every element as float64 / int64: the two truncation orders of the docstring, 0 where the
    element is not valid; an order too large for an int64 (an infinite ``x``) is stored as 2**62."""
    x = np.asarray(x, dtype=np.float64)
    m = np.asarray(m, dtype=np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (x > 0) & (m.imag >= 0) & ~np.isnan(m.real)
        xs = np.where(valid, x, 1.0)
        ay = np.where(valid, np.abs(m * xs), 1.0)
        nstop = np.floor(xs + 4.0 * np.cbrt(xs) + 2.0)
        nmx = np.floor(np.maximum(nstop, ay) + 15.0 + 8.0 * np.cbrt(ay))
        big = ~(nmx < 2.0 ** 62)
        nstop, nmx = (np.where(big, 2.0 ** 62, v) for v in (nstop, nmx))
    return valid, np.where(valid, nstop, 0).astype(np.int64), np.where(valid, nmx, 0).astype(np.int64)


def _checked(x, m):
    x, m = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(m, dtype=np.complex128))
    shape = x.shape
    x, m = np.ascontiguousarray(x).reshape(-1), np.ascontiguousarray(m).reshape(-1)
    valid, nstop, nmx = _orders(x, m)
    return shape, x, m, valid, nstop, nmx


def mie_efficiencies_numpy(x, m):
    """``(qext, qscat, cos_qscat)`` of the module docstring's algorithm in numpy, for arrays ``x`` and ``m`` of any common
    shape: the statement the device kernel is held to, and the host's way to the same numbers.  The elements are taken in
    groups of similar ``nmx`` so that one numpy step serves a whole group; an element's value depends on itself alone."""
    shape, x, m, valid, nstop, nmx = _checked(x, m)
    if nmx.size and nmx.max() > NMX_CAP:
        raise ValueError("mie_efficiencies_numpy: a series of %d terms (x = %r); at most %d are taken"
                         % (nmx.max(), float(x[np.argmax(nmx)]), NMX_CAP))
    out = np.full((3, x.size), np.nan)
    order = np.argsort(-nmx, kind="stable")
    order = order[valid[order]]
    for lo in range(0, order.size, _WAVE):
        idx = order[lo:lo + _WAVE]
        out[:, idx] = _series(x[idx], m[idx], nstop[idx], nmx[idx])
    return tuple(o.reshape(shape) for o in out)


def _series(x, m, nstop, nmx):
    """The series for a group of valid elements sorted by ``nmx``, largest first."""
    y = m * x
    top, ntop = int(nmx[0]), int(nstop.max())
    dy = np.zeros((ntop + 1, x.size), dtype=np.complex128)          # D_n(y), D_n(x) for n <= the group's largest nstop
    dx = np.zeros((ntop + 1, x.size))
    cy, cx = np.zeros(x.size, dtype=np.complex128), np.zeros(x.size)
    started = np.searchsorted(-nmx, -np.arange(top + 1), side="right")          # elements with nmx >= n
    with np.errstate(all="ignore"):
        for n in range(top, 0, -1):                                 # D_{n-1} from D_n, for the elements that have begun
            k = started[n]
            ny, nx = n / y[:k], n / x[:k]
            cy[:k] = ny - 1.0 / (cy[:k] + ny)
            cx[:k] = nx - 1.0 / (cx[:k] + nx)
            if n - 1 <= ntop:
                dy[n - 1, :k], dx[n - 1, :k] = cy[:k], cx[:k]
        psi1, chi1, chi2 = np.sin(x), np.cos(x), -np.sin(x)         # psi_{n-1}, chi_{n-1}, chi_{n-2}
        a1, b1 = np.zeros(x.size, dtype=np.complex128), np.zeros(x.size, dtype=np.complex128)
        qext, qsca, gqsc = np.zeros(x.size), np.zeros(x.size), np.zeros(x.size)
        for n in range(1, ntop + 1):
            live = n <= nstop
            nx = n / x
            psi = psi1 / (dx[n] + nx)
            chi = (2 * n - 1) / x * chi1 - chi2
            xi, xi1 = psi - 1j * chi, psi1 - 1j * chi1
            ca, cb = dy[n] / m + nx, m * dy[n] + nx
            an = (ca * psi - psi1) / (ca * xi - xi1)
            bn = (cb * psi - psi1) / (cb * xi - xi1)
            qext = np.where(live, qext + (2 * n + 1) * (an + bn).real, qext)
            qsca = np.where(live, qsca + (2 * n + 1) * ((an.real * an.real + an.imag * an.imag) + (bn.real * bn.real + bn.imag * bn.imag)), qsca)
            gqsc = np.where(live, gqsc + ((2 * n + 1) / (n * (n + 1)) * (an * np.conj(bn)).real
                                          + (n - 1) * (n + 1) / n * (a1 * np.conj(an) + b1 * np.conj(bn)).real), gqsc)
            psi1, chi2, chi1, a1, b1 = psi, chi1, chi, an, bn
    x2 = x * x
    return np.array([2.0 / x2 * qext, 2.0 / x2 * qsca, 4.0 / x2 * gqsc])


def _chunks(nstop_sorted, budget):
    """``[(first wave, past the last wave, bytes of scratch)]``: whole waves of 64 neighbours of the sorted list, as many per
    chunk as stay under ``budget`` bytes and never fewer than one."""
    n = nstop_sorted.size
    nwave = -(-n // _WAVE)
    rows = np.zeros(nwave * _WAVE, dtype=np.int64)
    rows[:n] = nstop_sorted
    wave_bytes = rows.reshape(nwave, _WAVE).max(axis=1) * (3 * _WAVE * 8)
    chunks, lo, used = [], 0, 0
    for w in range(nwave):
        if w > lo and used + wave_bytes[w] > budget:
            chunks.append((lo, w, used))
            lo, used = w, 0
        used += int(wave_bytes[w])
    chunks.append((lo, nwave, used))
    return chunks


def mie_efficiencies(x, m, ctx=None, _scratch_bytes=None):
    """``(qext, qscat, cos_qscat)`` of the module docstring's algorithm on the GPU (``picaso_mie_q_dev``, csrc/mie.hip), for
    arrays ``x`` and ``m`` of any common shape and any length.  The list is sorted by ``nmx`` (largest first), waves of 64
    neighbours are packed from it, and the waves run in chunks whose scratch (``3 * 64 * 8`` bytes per wave and term up to
    the wave's largest ``nstop``) stays under ``SCRATCH_BYTES``; a wave that needs more on its own gets what it needs.
    An element's bits do not depend on the list it came in or on the chunks."""
    global MIE_LAUNCHES
    from . import _lib
    from .device import DeviceArray
    shape, x, m, valid, nstop, nmx = _checked(x, m)
    n = x.size
    out = np.full((3, n), np.nan)
    if n == 0:
        return tuple(o.reshape(shape) for o in out)
    budget = SCRATCH_BYTES if _scratch_bytes is None else int(_scratch_bytes)
    order = np.argsort(-nmx, kind="stable")
    xs, mre, mim = x[order], np.ascontiguousarray(m.real[order]), np.ascontiguousarray(m.imag[order])
    ns, nm = (np.ascontiguousarray(np.minimum(v[order], 2 ** 31 - 1).astype(np.int32)) for v in (nstop, nmx))
    chunks = _chunks(ns, budget)
    with _lib.CALL_LOCK:
        ctx = ctx if ctx is not None else _lib.context()
        capped = int(nm[0]) > NMX_CAP                 # the C layer refuses it: no scratch is sized from such a count
        scratch = None if capped else DeviceArray((max(1, max(c[2] for c in chunks) // 8),), ctx)
        for first, last, need in chunks:
            a, b = first * _WAVE, min(n, last * _WAVE)
            d_out = DeviceArray((3, b - a), ctx)
            _lib.check(_lib.load().picaso_mie_q_dev(ctx, b - a, _lib.addr(xs[a:b]), _lib.addr(mre[a:b]), _lib.addr(mim[a:b]),
                                                    _lib.addr(ns[a:b]), _lib.addr(nm[a:b]),
                                                    None if capped else scratch.addr, 0 if capped else scratch.nbytes,
                                                    d_out.addr), ctx)
            MIE_LAUNCHES += 1
            out[:, order[a:b]] = d_out.to_host()
    return tuple(o.reshape(shape) for o in out)


# ---------------------------------------------------------------------------------------------------- the table
_tables = {}            # (pid, context, digest) -> the table's three arrays in HBM: content-addressed, oldest out first
_TABLES_MAX = 16


def _drop_context(value):
    for k in [k for k in _tables if k[1] == value]:
        _tables.pop(k)


def _register_hooks():
    from . import _lib
    _lib.on_context_destroy(_drop_context)


_register_hooks()


class MieTable:
    """Mie efficiencies per (wavelength, radius): what the reference's ``vj.get_mie`` returns as a six-tuple, under the names
    ``Parameterize`` keeps them by.  ``qext``, ``qscat``, ``cos_qscat`` (= g Qsca): ``(nwave, nradii)``; ``radius``:
    ``(nradii,)`` in cm; ``wave_in``: ``(nwave, nradii)`` in micron (a ``(nwave,)`` vector is repeated for every radius);
    ``area = PI * radius**2``.  The rows are stored WAVENUMBER INCREASING whatever order they arrive in -- the order of every
    cloud table of this package -- so that every consumer agrees on the grid.  ``tuple(table)`` is the reference's
    ``(qext, qscat, cos_qscat, nwave, radius, wave_in)``."""

    def __init__(self, qext, qscat, cos_qscat, radius, wave_in):
        radius = np.ascontiguousarray(radius, dtype=np.float64).reshape(-1)
        q = [np.asarray(a, dtype=np.float64) for a in (qext, qscat, cos_qscat)]
        wave_in = np.asarray(wave_in, dtype=np.float64)
        if wave_in.ndim == 1:
            wave_in = np.repeat(wave_in[:, None], radius.size, axis=1)
        if any(a.shape != wave_in.shape for a in q) or wave_in.ndim != 2 or wave_in.shape[1] != radius.size:
            raise ValueError("MieTable: qext, qscat, cos_qscat and wave_in are (nwave, nradii) and radius (nradii,); got %s, "
                             "%s and %s" % ([a.shape for a in q], wave_in.shape, radius.shape))
        rows = np.argsort(-wave_in[:, 0], kind="stable")
        self.qext, self.qscat, self.cos_qscat = (np.ascontiguousarray(a[rows]) for a in q)
        self.wave_in = np.ascontiguousarray(wave_in[rows])
        self.radius = radius
        self.nwave, self.nradii = self.wave_in.shape
        self.area = PI * radius ** 2
        self.wavenumber = 1e4 / self.wave_in[:, 0]
        self._digest = None

    def __iter__(self):
        return iter((self.qext, self.qscat, self.cos_qscat, self.nwave, self.radius, self.wave_in))

    @property
    def digest(self):
        if self._digest is None:
            from .optics import content_digest
            self._digest = tuple(content_digest(a) for a in (self.qext, self.qscat, self.cos_qscat, self.radius, self.wave_in))
        return self._digest

    def resident(self, ctx=None):
        """The three tables in HBM on ``ctx`` as one ``(3, nradii, nwave)`` DeviceArray (the wavelength index fastest: a
        wave's lanes read neighbours), uploaded once per context and content."""
        global TABLE_UPLOADS
        from . import _lib
        from .device import DeviceArray
        ctx = ctx if ctx is not None else _lib.context()
        key = (os.getpid(), getattr(ctx, "value", ctx), self.digest)
        hit = _tables.get(key)
        if hit is None:
            while len(_tables) >= _TABLES_MAX:
                _tables.pop(next(iter(_tables)))
            stack = np.stack([a.T for a in (self.qext, self.qscat, self.cos_qscat)])
            hit = _tables[key] = DeviceArray.from_host(stack, ctx)
            TABLE_UPLOADS += 1
        return hit


def default_edges(radius_cm):
    """Bin edges of a radius grid: the geometric means of neighbouring radii, mirrored (in log radius) at both ends."""
    r = np.asarray(radius_cm, dtype=np.float64).reshape(-1)
    if r.size < 2:
        raise ValueError("compute_mieff: one radius has no neighbours to take bin edges from: give edges_cm, or nsub=1")
    edges = np.empty(r.size + 1)
    edges[1:-1] = np.sqrt(r[:-1] * r[1:])
    edges[0] = r[0] * r[0] / edges[1]
    edges[-1] = r[-1] * r[-1] / edges[-2]
    return edges


def sub_radii(radius_cm, edges_cm=None, nsub=6):
    """``(nradii, nsub)`` radii the efficiencies of every bin are averaged over: ``lo + (hi - lo) * j / (nsub - 1)`` for the
    bin's edges ``lo, hi``; ``nsub = 1``: the radius itself."""
    r = np.asarray(radius_cm, dtype=np.float64).reshape(-1)
    nsub = int(nsub)
    if nsub < 1:
        raise ValueError("compute_mieff: nsub must be at least 1, got %d" % nsub)
    if nsub == 1:
        return r[:, None].copy()
    edges = default_edges(r) if edges_cm is None else np.asarray(edges_cm, dtype=np.float64).reshape(-1)
    if edges.size != r.size + 1:
        raise ValueError("compute_mieff: %d radii take %d edges, got %d" % (r.size, r.size + 1, edges.size))
    lo, hi = edges[:-1, None], edges[1:, None]
    return lo + (hi - lo) * np.arange(nsub)[None, :] / (nsub - 1)


def sub_mean(q):
    """The left-to-right sum over the last axis divided by its length."""
    acc = q[..., 0].copy()
    for j in range(1, q.shape[-1]):
        acc = acc + q[..., j]
    return acc / q.shape[-1]


def compute_mieff(wave_um, nn, kk, radius_cm, edges_cm=None, nsub=6, ctx=None, efficiencies=None):
    """The Mie table of a material with refractive index ``nn + i kk`` at the wavelengths ``wave_um`` (micron) for the radii
    ``radius_cm``: every efficiency the mean over ``nsub`` radii across the radius bin (``sub_radii``), which smooths the
    resonances of a single radius.  All ``nwave * nradii * nsub`` series go through ONE ``mie_efficiencies`` call with
    ``x = 2 PI r / (wave_um * 1e-4)``; the mean is a host step on the small result.  ``efficiencies``: another function of
    ``(x, m)`` in its place (``mie_efficiencies_numpy``: the same table without a GPU, slowly).  Returns a ``MieTable``."""
    wave = np.asarray(wave_um, dtype=np.float64).reshape(-1)
    m = np.asarray(nn, dtype=np.float64).reshape(-1) + 1j * np.asarray(kk, dtype=np.float64).reshape(-1)
    if m.size != wave.size:
        raise ValueError("compute_mieff: %d wavelengths and %d refractive indices" % (wave.size, m.size))
    radius = np.asarray(radius_cm, dtype=np.float64).reshape(-1)
    sub = sub_radii(radius, edges_cm, nsub)
    x = 2 * PI * sub[None, :, :] / (wave * 1e-4)[:, None, None]
    if efficiencies is None:
        q = mie_efficiencies(x, m[:, None, None], ctx=ctx)
    else:
        q = efficiencies(x, m[:, None, None])
    return MieTable(*(sub_mean(a) for a in q), radius, wave)


def write_mieff(path, table):
    """Write ``table`` as a ``.mieff`` text file, every number with ``repr``'s digits (the round trip is exact).  The
    layout is that of virga's files AS REMEMBERED -- virga was not at hand to confirm it:

        nwave nradii
        radius_cm                                   \\
        wavelength_micron qscat qext cos_qscat       |  nradii times
        ... (nwave lines)                           /

    Rows go out in the table's order (wavenumber increasing)."""
    with open(path, "w") as fh:
        fh.write("%d %d\n" % (table.nwave, table.nradii))
        for i in range(table.nradii):
            fh.write("%r\n" % float(table.radius[i]))
            for w in range(table.nwave):
                fh.write("%r %r %r %r\n" % (float(table.wave_in[w, i]), float(table.qscat[w, i]), float(table.qext[w, i]),
                                            float(table.cos_qscat[w, i])))


def read_mieff(path):
    """Read a ``.mieff`` file (layout: ``write_mieff``) structurally: after the two counts of the first line, a line of one
    number opens a radius and a line of four numbers is a row of it; anything else, or counts that disagree with what was
    read, is an error that names the line -- never a silent mis-parse.  Rows may come in either wavelength order."""
    radii, blocks, header = [], [], None
    with open(path) as fh:
        for lineno, line in enumerate(fh, 1):
            words = line.split()
            if not words:
                continue
            try:
                if header is None:
                    if len(words) != 2:
                        raise ValueError
                    header = (int(words[0]), int(words[1]))
                    continue
                vals = [float(v) for v in words]
            except ValueError:
                raise ValueError("%s:%d: not a .mieff line (the first holds 'nwave nradii', the others one radius or "
                                 "'wavelength qscat qext cos_qscat'): %r" % (path, lineno, line.strip())) from None
            if len(vals) == 1:
                radii.append(vals[0])
                blocks.append([])
            elif len(vals) == 4 and blocks:
                blocks[-1].append(vals)
            else:
                raise ValueError("%s:%d: a line of %d numbers; a radius is one number, a row is four and follows a radius"
                                 % (path, lineno, len(vals)))
    if header is None:
        raise ValueError("%s: empty file" % path)
    nwave, nradii = header
    if len(radii) != nradii or any(len(b) != nwave for b in blocks):
        raise ValueError("%s: the header announces %d wavelengths x %d radii, the file holds %d radii with %s rows"
                         % (path, nwave, nradii, len(radii), sorted({len(b) for b in blocks})))
    data = np.array(blocks, dtype=np.float64).reshape(nradii, nwave, 4)
    return MieTable(data[:, :, 2].T, data[:, :, 1].T, data[:, :, 3].T, radii, data[:, :, 0].T)


def get_mie(gas, directory):
    """The table of ``directory/<gas>.mieff`` (the reference's ``vj.get_mie(gas, directory=...)``) as a ``MieTable``."""
    return read_mieff(os.path.join(directory, "%s.mieff" % gas))


def read_refrind(path):
    """``(wave_um, n, k)`` of a refractive-index file: whitespace-separated columns ``wave n k`` or ``index wave n k``;
    empty lines and lines that begin with ``#`` are skipped."""
    rows = []
    with open(path) as fh:
        for lineno, line in enumerate(fh, 1):
            words = line.split()
            if not words or words[0].startswith("#"):
                continue
            try:
                vals = [float(v) for v in words]
            except ValueError:
                raise ValueError("%s:%d: not numbers: %r" % (path, lineno, line.strip())) from None
            if len(vals) not in (3, 4) or (rows and len(vals) != len(rows[0])):
                raise ValueError("%s:%d: %d columns; 'wave n k' or 'index wave n k' throughout" % (path, lineno, len(vals)))
            rows.append(vals)
    if not rows:
        raise ValueError("%s: no rows" % path)
    a = np.array(rows, dtype=np.float64)[:, -3:]
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


# ---------------------------------------------------------------------------------------------------- size distributions
_NAN_LOGNORM = {"sigma": np.nan, "lograd": np.nan}
_NAN_HANSEN = {"b": np.nan, "lograd": np.nan}
_NAN_SLAB = {"ptop": np.nan, "dp": np.nan, "reference_tau": np.nan}
_NAN_DECK = {"ptop": np.nan, "dp": np.nan}


def _dist_scalars(distribution, lognorm_kwargs, hansen_kwargs):
    """The numbers a distribution is made of, each formed as reference parameterizations.py:64-78 forms it:
    ``('lognorm', 1/(sigma sqrt(2 pi)), lograd, 2 sigma**2)`` or ``('hansen', (1 - 3b)/b, a b)``."""
    if "lognorm" in distribution:
        sigma = lognorm_kwargs["sigma"]
        lograd = lognorm_kwargs["lograd"]
        if np.isnan(sigma):
            raise Exception("lognorm_kwargs have not been defined")
        return "lognorm", 1 / (sigma * np.sqrt(2 * np.pi)), lograd, 2 * sigma ** 2
    if "hansen" in distribution:
        a = 10 ** hansen_kwargs["lograd"]
        b = hansen_kwargs["b"]
        return "hansen", (1 - 3 * b) / b, a * b
    raise Exception("Only lognormal and hansen distributions available")


def _lognorm(logradius, c, lograd, two_sigma_sq):
    return c * np.exp(-(logradius - lograd) ** 2 / two_sigma_sq)


def _hansen(radius, ten_r, power, ab):
    # (np.power with an array exponent: the ``**`` of an array with a scalar 1, 2, 0.5 or -1 takes a shortcut that a batch's
    # array of exponents does not, and both ways must give the same bits)
    return np.power(ten_r, power + 0 * radius) * np.exp(-radius / ab)


def get_particle_dist(radius, distribution, lognorm_kwargs=_NAN_LOGNORM, hansen_kwargs=_NAN_HANSEN):
    """The particle-size distribution at ``radius`` (cm) of reference parameterizations.py:59-80, literally: ``'lognorm'``
    ``1/(sigma sqrt(2 pi)) exp(-(log10 r - lograd)**2 / (2 sigma**2))``; ``'hansen'`` the expression AS WRITTEN THERE,
    ``(10**r)**((1 - 3b)/b) exp(-r/(a b))`` with ``a = 10**lograd``; its two exceptions."""
    radius = np.asarray(radius, dtype=np.float64)
    sc = _dist_scalars(distribution, lognorm_kwargs, hansen_kwargs)
    if sc[0] == "lognorm":
        return _lognorm(np.log10(radius), *sc[1:])
    return _hansen(radius, 10 ** radius, *sc[1:])


def calc_optics_user_r_dist(wave_in, ndz, radius, r_distribution, qext, qscat, cos_qscat):
    """Optical depth, single-scattering albedo and asymmetry per wavelength of ``ndz`` particles per cm2 with the size
    distribution ``r_distribution`` over the table's radii (cm):

        wgt[r] = (ndz * (PI * radius[r]**2)) * r_distribution[r]
        opd, opd_scat, opd_cos = the left-to-right sums over r, from 0, of qext, qscat, cos_qscat[w, r] * wgt[r]
        w0 = opd_scat / opd where opd > 0, else 0;   g0 = opd_cos / opd_scat where opd_scat > 0, else 0

    every product rounded, nothing fused.  Returns ``opd, w0, g0, 1e4 / wave_in[:, 0]``.  This is THIS PACKAGE's statement of
    what the reference's ``vj.calc_optics_user_r_dist(wave_in, ndz, radius, u.cm, ...)`` computes (virga was not at hand;
    there is no astropy unit argument: the radius is in cm).  It is kept in this one function so that it can be pinned to
    virga's own the day virga is at hand."""
    wave_in, qext, qscat, cos_qscat = (np.asarray(a, dtype=np.float64) for a in (wave_in, qext, qscat, cos_qscat))
    radius = np.asarray(radius, dtype=np.float64)
    wgt = (ndz * (PI * radius ** 2)) * np.asarray(r_distribution, dtype=np.float64)
    opd, opd_scat, opd_cos = (np.zeros(qext.shape[0]) for _ in range(3))
    for r in range(radius.size):
        opd = opd + qext[:, r] * wgt[r]
        opd_scat = opd_scat + qscat[:, r] * wgt[r]
        opd_cos = opd_cos + cos_qscat[:, r] * wgt[r]
    with np.errstate(divide="ignore", invalid="ignore"):
        w0 = np.where(opd > 0, opd_scat / opd, 0.0)
        g0 = np.where(opd_scat > 0, opd_cos / opd_scat, 0.0)
    return opd, w0, g0, 1e4 / wave_in[:, 0]


# ---------------------------------------------------------------------------------------------------- the two cloud forms
def cloud_brewster_mie(param, table, distribution, decay_type, lognorm_kwargs=_NAN_LOGNORM, hansen_kwargs=_NAN_HANSEN,
                       slab_kwargs=_NAN_SLAB, deck_kwargs=_NAN_DECK):
    """``Parameterize.cloud_brewster_mie`` of the reference (parameterizations.py:148-198) for the pressure grid of ``param``
    and the Mie table ``table`` in place of the condensate's name: the table summed over the size distribution for ONE
    particle per cm2, its optical depth scaled to 1 at its largest and laid on the slab or deck profile.  Returns the
    reference's DataFrame."""
    from .parameterizations import picaso_format
    dist = get_particle_dist(table.radius, distribution, lognorm_kwargs, hansen_kwargs)
    opd, w0, g0, wavenumber_grid = calc_optics_user_r_dist(table.wave_in, 1, table.radius, dist, table.qext, table.qscat,
                                                           table.cos_qscat)
    opd_profile = param._grey_layers(decay_type, slab_kwargs, deck_kwargs)
    with np.errstate(divide="ignore", invalid="ignore"):
        return picaso_format(opd, w0, g0, wavenumber_grid, param.pressure_layer, opd_profile=opd_profile)


def _fsed_decay(pressure_layer, base_pressure, fsed):
    """``opd_h`` of reference parameterizations.py:129-141: 10 exp(-fsed z / 10) at and above the base, 0 below it, over
    its largest value."""
    scale_h = 10
    z = np.linspace(100, 0, len(pressure_layer))
    opd_h = pressure_layer * 0 + 10
    opd_h[base_pressure < pressure_layer] = 0
    above = base_pressure >= pressure_layer
    opd_h[above] = opd_h[above] * np.exp(-fsed * z[above] / scale_h)
    with np.errstate(divide="ignore", invalid="ignore"):
        return opd_h / np.max(opd_h)


def cloud_flex_fsed(param, table, base_pressure, ndz, fsed, distribution, lognorm_kwargs=_NAN_LOGNORM,
                    hansen_kwargs=_NAN_HANSEN):
    """``Parameterize.cloud_flex_fsed`` of the reference (parameterizations.py:94-146) for the pressure grid of ``param`` and
    the Mie table ``table``: ``ndz`` particles per cm2 with the size distribution, falling off above ``base_pressure`` (bar)
    as ``exp(-fsed z / 10)``, nothing below it.  Returns the reference's DataFrame."""
    from .parameterizations import picaso_format
    dist = get_particle_dist(table.radius, distribution, lognorm_kwargs, hansen_kwargs)
    opd, w0, g0, wavenumber_grid = calc_optics_user_r_dist(table.wave_in, ndz, table.radius, dist, table.qext, table.qscat,
                                                           table.cos_qscat)
    opd_h = _fsed_decay(param.pressure_layer, base_pressure, fsed)
    with np.errstate(divide="ignore", invalid="ignore"):
        return picaso_format(opd, w0, g0, wavenumber_grid, param.pressure_layer, p_bottom=base_pressure, p_decay=opd_h)


flex_cloud = cloud_flex_fsed


# ---------------------------------------------------------------------------------------------------- the batch
_KINDS = {"brewster_mie": 0, "flex_fsed": 1}


def _batch_records(param, samples, average=None):
    """The launch's host half: every discrete decision and everything small.  Returns ``(tables, deck_table (S, K),
    deck_kind (S, K), wgt (S, K, rmax), factor (S, K, nlayer), inside (S, K, nlayer), average, per-sample stamps)``."""
    S = len(samples)
    K = max(len(s) for s in samples)
    if min(len(s) for s in samples) < 1 or K > 4:
        raise ValueError("cloud_tables_batch: every sample takes 1 to 4 decks")
    average = int(K > 1) if average is None else int(bool(average))
    if not average and K != 1:
        raise ValueError("cloud_tables_batch: average=0 takes one deck per sample")
    nlayer, player = param.nlayer, param.pressure_layer
    tables, where = [], {}
    deck_table, deck_kind = np.full((S, K), -1, dtype=np.int32), np.zeros((S, K), dtype=np.int32)
    groups = {}                                        # (table, distribution form) -> [(s, k, scalars)]
    flex, stamps = [], [[None] * len(s) for s in samples]
    factor, inside = np.zeros((S, K, nlayer)), np.zeros((S, K, nlayer))
    ndz = np.ones((S, K))
    for s, sample in enumerate(samples):
        for k, deck in enumerate(sample):
            kind, table = deck.get("kind"), deck.get("table")
            if kind not in _KINDS or not isinstance(table, MieTable):
                raise Exception("cloud_tables_batch: a deck takes kind = 'brewster_mie' or 'flex_fsed' and table = a MieTable, "
                                "got %r and %r" % (kind, type(table).__name__))
            t = where.get(id(table))
            if t is None:
                if tables and not np.array_equal(table.wave_in[:, 0], tables[0].wave_in[:, 0]):
                    raise ValueError("cloud_tables_batch: every table of a call shares one wavelength grid")
                t = where[id(table)] = len(tables)
                tables.append(table)
            deck_table[s, k], deck_kind[s, k] = t, _KINDS[kind]
            sc = _dist_scalars(deck["distribution"], deck.get("lognorm_kwargs", _NAN_LOGNORM),
                               deck.get("hansen_kwargs", _NAN_HANSEN))
            groups.setdefault((t, sc[0]), []).append((s, k, sc[1:]))
            if kind == "brewster_mie":
                factor[s, k] = param._grey_layers(deck["decay_type"], deck.get("slab_kwargs", _NAN_SLAB),
                                                  deck.get("deck_kwargs", _NAN_DECK))
                inside[s, k] = 1.0
                kw = deck.get("slab_kwargs", _NAN_SLAB) if deck["decay_type"] == "slab" else deck.get("deck_kwargs", _NAN_DECK)
                par = (float(deck["decay_type"] == "slab"),) + tuple(float(kw[key]) for key in sorted(kw))
            else:
                flex.append((s, k, deck["base_pressure"], deck["fsed"]))
                ndz[s, k] = deck["ndz"]
                par = (float(deck["base_pressure"]), float(deck["ndz"]), float(deck["fsed"]))
            stamps[s][k] = (float(_KINDS[kind]), table.digest, sc[0]) + tuple(float(v) for v in sc[1:]) + par
    if flex:                                           # reference :129-141 and picaso_format's own division, all decks at once
        fs, fk = (np.array([f[j] for f in flex]) for j in (0, 1))
        base, fsed = (np.array([f[j] for f in flex], dtype=np.float64)[:, None] for j in (2, 3))
        z = np.linspace(100, 0, nlayer)[None, :]
        above = base >= player[None, :]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            opd_h = np.where(above, (player * 0 + 10)[None, :] * np.exp(-fsed * z / 10), 0.0)
            opd_h = opd_h / np.max(opd_h, axis=1)[:, None]
            factor[fs, fk] = opd_h / np.max(opd_h, axis=1)[:, None]
        inside[fs, fk] = ((1e-10 <= player[None, :]) & (player[None, :] <= base)).astype(np.float64)
    rmax = max(t.nradii for t in tables)
    wgt = np.zeros((S, K, rmax))
    for (t, form), members in groups.items():          # the distribution of every deck of a table in one expression
        table = tables[t]
        gs, gk = (np.array([g[j] for g in members]) for j in (0, 1))
        cols = [np.array([g[2][j] for g in members], dtype=np.float64)[:, None] for j in range(len(members[0][2]))]
        with np.errstate(all="ignore"):
            if form == "lognorm":
                dist = _lognorm(np.log10(table.radius)[None, :], *cols)
            else:
                dist = _hansen(table.radius[None, :], (10 ** table.radius)[None, :], *cols)
            wgt[gs, gk, :table.nradii] = (ndz[gs, gk][:, None] * table.area[None, :]) * dist
    return tables, deck_table, deck_kind, wgt, factor, inside, average, [tuple(s) for s in stamps]


def _resident_grid(param, table, ctx):
    """Per ``Parameterize`` and context: the tables' wavenumber grid in HBM with the digests the stamps carry -- the record
    ``Parameterize._resident_grids`` keeps for the 196-point grid, for this one."""
    from . import _lib
    from .device import DeviceArray
    from .optics import content_digest
    ctx = ctx if ctx is not None else _lib.context()
    grid = np.ascontiguousarray(table.wavenumber, dtype=np.float64)
    key = getattr(ctx, "value", ctx)
    memo = param.__dict__.setdefault("_mie_resident", {})
    hit = memo.get(key)
    if hit is None or hit["pressure"] is not param.pressure_level or not np.array_equal(hit["grid"], grid):
        hit = memo[key] = dict(ctx=ctx, grid=grid, pressure=param.pressure_level, d_xp=DeviceArray.from_host(grid, ctx),
                               device=_lib.device_of(ctx), digest=(content_digest(param.pressure_level), content_digest(grid)))
    return hit


def cloud_tables_batch(param, samples, average=None, ctx=None):
    """The Mie cloud tables of ``S`` samples in ONE call of ``picaso_mie_cloud_tables_dev`` (csrc/miecloud.hip).  ``samples``:
    ``S`` lists of 1 to 4 decks, each the keyword dictionary of ``cloud_brewster_mie`` or ``cloud_flex_fsed`` with the keys
    ``kind`` (``'brewster_mie'`` / ``'flex_fsed'``) and ``table`` (a ``MieTable``; every table of a call on one wavelength
    grid).  ``average`` as in ``Parameterize.cloud_tables_batch``: 1 combines a sample's decks with the arithmetic of
    ``cloud_averaging``, 0 stores its one deck as it is; default 1 when a sample has more than one deck.  The host takes the
    discrete decisions and forms what is small (layer factors, masks, the distributions of the whole batch at once); the
    device sums the tables over the distributions and writes the ``(S, 3, nlayer, nwave)`` rows -- bit for bit those of the
    host functions.  Returns ``S`` ``ParamCloudTable`` on the tables' grid: ``inputs.clouds(df=...)``, ``spectrum``,
    ``spectrum_async`` and ``spectrum_batch`` read them where they lie."""
    global LAUNCHES
    from . import _lib, device
    from .device import DeviceArray
    from .parameterizations import ParamCloudTable
    S = len(samples)
    if S == 0:
        return []
    tables, deck_table, deck_kind, wgt, factor, inside, average, stamps = _batch_records(param, samples, average)
    K, nlayer, nwave, rmax = deck_table.shape[1], param.nlayer, tables[0].nwave, wgt.shape[2]
    with _lib.CALL_LOCK:
        res = _resident_grid(param, tables[0], ctx)
        ctx = res["ctx"]
        d_tables = [t.resident(ctx) for t in tables]
        nradii = np.array([t.nradii for t in tables], dtype=np.int32)
        d_wgt, d_factor, d_inside = (DeviceArray.from_host(a, ctx) for a in (wgt, factor, inside))
        work = DeviceArray((S * K * (3 * nwave + 1),), ctx)
        out = DeviceArray((S, 3 * nlayer, nwave), ctx)
        _lib.check(_lib.load().picaso_mie_cloud_tables_dev(
            ctx, S, K, nlayer, nwave, average, len(tables), _lib.ptr_array(d_tables), _lib.addr(nradii),
            _lib.addr(np.ascontiguousarray(deck_table)), _lib.addr(np.ascontiguousarray(deck_kind)), rmax, d_wgt.addr,
            d_factor.addr, d_inside.addr, work.addr, out.addr), ctx)
        LAUNCHES += 1
        device.sync(ctx)
    return [ParamCloudTable(res, param.pressure_layer, out.row_block(s), nlayer, res["digest"] + (average, stamps[s]))
            for s in range(S)]
