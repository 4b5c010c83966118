"""Generate tests/golden/attenuation.npz by running the REFERENCE's own source (build container only):

    python tests/golden/make_attenuation.py

``justplotit.photon_attenuation`` (reference justplotit.py:426-536), ``taumap`` (:1019-1131), ``heatmap_taus`` (:1284-1323)
and the ``np.mean`` lines of ``all_optics_1d`` (:1197-1282) on synthetic ``full_output`` dictionaries.  The figures are
drawn on recording stubs: what the reference hands to ``pcolormesh``, ``scatter`` and ``line`` is what is stored.

Scenes.  ``s13``, ``s3``, ``s2``: 150 wavenumbers (two full 64-lane tiles and a partial one, with a gap and an isolated
point so that R = 60 leaves bins empty) and 13, 3 and 2 levels; ``ck13``: 13 levels and three Gauss points with a
``taugas`` that differs per Gauss point; ``map``: a 3-D scene of 3 x 2 facets, 5 levels, two Gauss points.  Deliberate
columns (``cols``): an all-zero cloud column, layers of zeros at the top (the leading zeros repeat), a ``dtau`` sequence of
0.25, 0.25, 0.5 in the gas and 0.25, 0.5, 0.5 in the Rayleigh plane (exact hits and exact ties around 0.5 and 1, and a
value that repeats down to the bottom), an opaque layer (1e4), a column whose total depth stays below every ``at_tau``
but 0, and one column with a NaN.  In ``map`` one facet has a cloud that is non-zero in every layer (the quirk of
:1082-1083), one has no cloud and one has a clear top.

Asserted: the walk down the column that csrc/attenuation.hip performs, restated here in numpy, gives the reference's
level on every column of every scene, ``at_tau`` and Gauss point except the NaN column -- exactly one column per scene --
and no scene holds a negative ``dtau``.  The file is written with fixed zip time stamps: a second run reproduces it byte
for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)

from make_contribfn import _justplotit  # noqa: E402

NWNO, R_BIN = 150, 60
AT_TAUS = (0.0, 0.5, 1.0, 1e6)
COLS = {"zero_cloud": 5, "opaque": 17, "top_zeros": 20, "ties": 70, "thin": 100, "nan": 131}
WINDOWS = ((4.3, 4.9), (3.6, 3.8), (3.75, 4.0), (3.0, 5.1))          # many columns, one, none, all
MAP_WNO = np.linspace(8000.0, 12500.0, 7)
MAP_WAVELENGTHS = (1.0, 1.2)
MAP_WINDOWS = ((0.85, 1.2), (0.0, 0.5))                               # five columns, none


class Recorder:
    """Stands in for a figure, an axis, pyplot: every attribute is a recorder, every call is kept."""

    def __init__(self, log=None, name=""):
        self.__dict__["_log"] = [] if log is None else log
        self.__dict__["_name"] = name

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Recorder(self._log, k)

    def __setattr__(self, k, v):
        pass

    def __call__(self, *a, **kw):
        self._log.append((self._name, a, kw))
        return Recorder(self._log, self._name + "()")

    def __getitem__(self, k):
        return self

    def calls(self, name):
        return [(a, kw) for n, a, kw in self._log if n == name]


def scene(nlevel, ngauss=1):
    """A ``full_output`` dictionary with the reference's keys, planes ``(nlayer, nwno, ngauss)``."""
    nlayer = nlevel - 1
    rng = np.random.default_rng(700 + 10 * nlevel + ngauss)
    wno = np.concatenate((np.linspace(2000.0, 2400.0, 99), [2700.0], np.linspace(3000.0, 3300.0, 50)))
    assert wno.size == NWNO
    plev = np.logspace(-5, 1.5, nlevel)
    play = np.sqrt(plev[1:] * plev[:-1])
    lam = (wno - wno[0]) / (wno[-1] - wno[0])
    depth = np.diff(plev)[:, None] / plev[-1]
    gas = 40.0 * depth ** 0.7 * 10.0 ** (1.2 * np.sin(7 * lam)[None, :] - 0.8) * rng.uniform(0.6, 1.4, (nlayer, NWNO))
    ray = 3.0 * depth * (wno[None, :] / 3300.0) ** 4
    cld = np.zeros((nlayer, NWNO))
    slab = slice(nlayer // 2, nlayer // 2 + max(1, nlayer // 4))
    cld[slab] = 0.9 * (1.0 + 0.4 * lam)[None, :]
    w0 = rng.uniform(0.3, 0.999, (nlayer, NWNO))
    g0 = rng.uniform(0.0, 0.9, (nlayer, NWNO))
    c = COLS
    cld[:, c["zero_cloud"]] = 0.0
    gas[nlayer // 3, c["opaque"]] = 1e4
    ntop = max(1, nlayer // 3) if nlayer > 1 else 0
    for a in (gas, cld, ray):
        a[:ntop, c["top_zeros"]] = 0.0
    gas[:, c["ties"]] = ([0.25, 0.25, 0.5] + [0.3] * nlayer)[:nlayer]
    ray[:, c["ties"]] = ([0.25, 0.5, 0.5] + [0.0] * nlayer)[:nlayer]
    cld[:, c["ties"]] = ([0.5, 0.5] + [0.0] * nlayer)[:nlayer]
    w0[:, c["ties"]] = 0.5                                                  # exact products: 0.25, 0.25, then zeros
    for a in (gas, cld, ray):
        a[:, c["thin"]] = 1e-3 * rng.uniform(0.1, 1.0, nlayer) / nlayer
    gas[min(1, nlayer - 1), c["nan"]] = np.nan
    per_gauss = 10.0 ** np.linspace(0.0, 1.5, ngauss) if ngauss > 1 else np.ones(1)
    taugas = gas[:, :, None] * per_gauss[None, None, :]
    if ngauss > 1:
        taugas = taugas * rng.uniform(0.8, 1.25, taugas.shape)
        taugas[:, c["ties"], :] = gas[:, c["ties"], None]
    over = lambda a: np.repeat(a[:, :, None], ngauss, axis=2)              # noqa: E731
    return {"wavenumber": wno, "taugas": taugas, "taucld": over(cld), "tauray": over(ray),
            "layer": {"pressure": play, "cloud": {"opd": cld.copy(), "w0": w0, "g0": g0}},
            "level": {"pressure": plev}}


def map_scene():
    """The dictionary of a 3-D run: planes ``(nlayer, nwno, ng, nt, ngauss)``, w0 ``(nlayer, nwno, ng, nt)``."""
    nlevel, ng, nt, ngauss, nwno = 5, 3, 2, 2, MAP_WNO.size
    nlayer = nlevel - 1
    rng = np.random.default_rng(4242)
    shape = (nlayer, nwno, ng, nt, ngauss)
    gas = rng.uniform(0.05, 0.6, shape) * np.array([1.0, 6.0])
    ray = rng.uniform(0.01, 0.4, shape[:4])
    cld = rng.uniform(0.2, 0.9, shape[:4])
    cld[:2, :, 0, 0] = 0.0                       # facet (0, 0): a clear top
    cld[:, :, 2, 1] = 0.0                        # facet (2, 1): no cloud
    # facet (1, 0) and the others: non-zero in every layer -- the cumulative column holds exactly one zero (the quirk)
    w0 = rng.uniform(0.4, 0.99, shape[:4])
    cld[2, :, 0, 0], w0[2, :, 0, 0] = 1.0, 0.5   # ... and reaches 0.5 exactly at level 3
    plev = np.logspace(-4, 1, nlevel)[:, None, None] * rng.uniform(0.8, 1.2, (1, ng, nt))
    over = lambda a: np.repeat(a[..., None], ngauss, axis=4)               # noqa: E731
    return {"wavenumber": MAP_WNO, "taugas": gas, "taucld": over(cld), "tauray": over(ray),
            "layer": {"pressure": np.sqrt(plev[1:] * plev[:-1]),
                      "cloud": {"opd": cld.copy(), "w0": w0, "g0": rng.uniform(0.0, 0.9, shape[:4])}},
            "level": {"pressure": plev},
            "latitude": np.array([-0.6, 0.6]), "longitude": np.array([-0.9, 0.0, 0.9])}


def walk(d, at_tau):
    """The level the kernel keeps for one column of layer depths ``d`` (csrc/attenuation.hip), -1 for a NaN column."""
    c = cb = 0.0
    best, gap = 0, abs(0.0 - at_tau)
    for i, v in enumerate(d):
        c = c + v
        g = abs(c - at_tau)
        if g < gap or c == cb:
            best, gap, cb = i + 1, g, c
    return -1 if c != c else best


def write_npz(path, store):
    """``np.savez_compressed`` with fixed time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(store[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def attenuation(jpi, full, tag, store, ngauss):
    nlayer, nwno = full["tauray"].shape[:2]
    plev = full["level"]["pressure"]
    excluded = set()
    for ig in range(ngauss):
        planes = (full["taugas"][:, :, ig], full["taucld"][:, :, ig] * full["layer"]["cloud"]["w0"], full["tauray"][:, :, ig])
        assert not any((p < 0).any() for p in planes), "negative dtau"
        for at in AT_TAUS:
            with np.errstate(all="ignore"):
                ret = jpi.photon_attenuation(full, at_tau=at, return_output=True, igauss=ig)
                ref_p = np.array(ret[2:5])
                ref_l = np.array([jpi.find_nearest_2d(np.concatenate((np.zeros((1, nwno)), np.cumsum(p, axis=0))), at)
                                  for p in planes]).astype(np.int32)
            assert np.array_equal(ret[1], 1e4 / full["wavenumber"])
            assert np.array_equal(plev[ref_l], ref_p, equal_nan=True)       # these ARE the indices behind the pressures
            mine = np.array([[walk(p[:, w], at) for w in range(nwno)] for p in planes])
            differ = np.flatnonzero((mine != ref_l).any(axis=0))
            excluded |= set(int(w) for w in differ) | set(int(w) for w in np.flatnonzero((mine < 0).any(axis=0)))
            ok = np.arange(nwno) != COLS["nan"]
            assert np.array_equal(mine[:, ok], ref_l[:, ok]), (tag, ig, at)
            store["%spa/%g/%d/pressure" % (tag, at, ig)] = ref_p
            store["%spa/%g/%d/level" % (tag, at, ig)] = ref_l
    assert excluded == {COLS["nan"]}, (tag, excluded)                        # a condition, not a measurement


def heatmaps(jpi, full, tag, store):
    out = {"wavenumber": full["wavenumber"], "full_output": full}
    for R in (0, R_BIN):
        rec = Recorder()
        real, jpi.plt = jpi.plt, rec
        try:
            with np.errstate(all="ignore"):
                jpi.heatmap_taus(out, R=R)
        finally:
            jpi.plt = real
        calls = rec.calls("pcolormesh")
        assert len(calls) == 3
        for k, (a, _) in zip(("taugas", "taucld", "tauray"), calls):
            store["%sheat/R%d/%s" % (tag, R, k)] = np.array(a[2])
        wno = full["wavenumber"]
        store["%sheat/R%d/wavenumber" % (tag, R)] = jpi.mean_regrid(wno, wno, R=R)[0] if R else wno
    z = store["%sheat/R%d/tauray" % (tag, R_BIN)]
    assert np.isnan(z).any(axis=0).any() and not np.isnan(z).all()          # R = 60 leaves bins empty
    assert (store["%sheat/R0/taucld" % tag] == -100).any()


def optics_means(jpi, full, tag, store, windows=WINDOWS, ng=None, nt=None):
    for i, win in enumerate(windows):
        rec = Recorder()
        real = jpi.figure, jpi.gridplot
        jpi.figure = jpi.gridplot = rec
        try:
            with np.errstate(all="ignore"):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    jpi.all_optics_1d(full, list(win), ng=ng, nt=nt, colors=["black"])
        finally:
            jpi.figure, jpi.gridplot = real
        lines = rec.calls("line")                                           # fopd, fg0, fssa in the reference's order
        assert len(lines) == 3
        for k, (a, _) in zip(("opd", "g0", "w0"), lines):
            store["%soptics/%d/%s" % (tag, i, k)] = np.array(a[0])
        wave = 1e4 / full["wavenumber"]
        store["%soptics/%d/count" % (tag, i)] = np.array(int(((wave > win[0]) & (wave < win[1])).sum()))
    if windows is WINDOWS:
        counts = [int(store["%soptics/%d/count" % (tag, i)]) for i in range(len(WINDOWS))]
        assert counts[1] == 1 and counts[2] == 0 and counts[3] == full["wavenumber"].size and counts[0] > 10, counts


def taumaps(jpi, full, store):
    nlayer, nwno, ng, nt, ngauss = full["taugas"].shape
    for wl in MAP_WAVELENGTHS:
        iw = int(jpi.find_nearest_1d(1e4 / full["wavenumber"], wl))
        store["map/iw/%g" % wl] = np.array(iw)
        for ig in range(ngauss):
            for at in AT_TAUS:
                rec = Recorder()
                real, jpi.plt = jpi.plt, rec
                try:
                    jpi.taumap(full, at_tau=at, wavelength=wl, igauss=ig)
                finally:
                    jpi.plt = real
                sc = rec.calls("scatter")
                assert len(sc) == 3
                maps = np.array([np.asarray(kw["c"]).reshape(nt, ng).T for _, kw in sc])
                # the figure-free lines restated with the kernel's walk, asserted against the run of the function
                plev = full["level"]["pressure"]
                mine = np.zeros((3, ng, nt))
                for g in range(ng):
                    for t in range(nt):
                        cols = (full["taugas"][:, iw, g, t, ig],
                                full["taucld"][:, iw, g, t, ig] * full["layer"]["cloud"]["w0"][:, iw, g, t],
                                full["tauray"][:, iw, g, t, ig])
                        assert not any((c_ < 0).any() for c_ in cols)
                        lv = [walk(c_, at) for c_ in cols]
                        if np.count_nonzero(np.concatenate(([0.0], np.cumsum(cols[1]))) == 0) == 1:
                            lv[1] = nlayer
                        mine[:, g, t] = [plev[l, g, t] for l in lv]
                assert np.array_equal(mine, maps), (wl, ig, at)
                store["map/taumap/%g/%d/%g" % (wl, ig, at)] = maps
    quirk = store["map/taumap/1/0/0.5"][1]
    assert quirk[1, 0] == full["level"]["pressure"][-1, 1, 0] and quirk[0, 0] != full["level"]["pressure"][-1, 0, 0]


def main():
    jpi = _justplotit()
    jpi.figure = jpi.Legend = Recorder()                    # photon_attenuation draws on these
    jpi.Colorblind8 = ["#000000"] * 8
    store = {"at_taus": np.array(AT_TAUS), "R": np.array(R_BIN), "windows": np.array(WINDOWS),
             "cols": np.array([COLS[k] for k in sorted(COLS)]), "col_names": np.array(sorted(COLS)),
             "scenes": np.array(["s13", "s3", "s2", "ck13"]), "map/wavelengths": np.array(MAP_WAVELENGTHS)}
    for name, nlevel, ngauss in (("s13", 13, 1), ("s3", 3, 1), ("s2", 2, 1), ("ck13", 13, 3)):
        full, tag = scene(nlevel, ngauss), name + "/"
        for k in ("taugas", "taucld", "tauray"):
            store[tag + k] = full[k]
        store[tag + "wno"] = full["wavenumber"]
        store[tag + "level/pressure"] = full["level"]["pressure"]
        store[tag + "layer/pressure"] = full["layer"]["pressure"]
        for k, v in full["layer"]["cloud"].items():
            if k == "w0" or name in ("s13", "s2"):              # opd and g0 only where all_optics_1d is run
                store[tag + "cloud/" + k] = v
        attenuation(jpi, full, tag, store, ngauss)
        heatmaps(jpi, full, tag, store)
        if name in ("s13", "s2"):
            optics_means(jpi, full, tag, store)
        print(name, "ok")
    full = map_scene()
    for k in ("taugas", "taucld", "tauray", "latitude", "longitude"):
        store["map/" + k] = full[k]
    store["map/wno"] = full["wavenumber"]
    store["map/level/pressure"] = full["level"]["pressure"]
    store["map/layer/pressure"] = full["layer"]["pressure"]
    for k, v in full["layer"]["cloud"].items():
        store["map/cloud/" + k] = v
    taumaps(jpi, full, store)
    store["map/windows"] = np.array(MAP_WINDOWS)
    optics_means(jpi, full, "map/f21/", store, windows=MAP_WINDOWS, ng=2, nt=1)
    path = os.path.join(HERE, "attenuation.npz")
    write_npz(path, store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
