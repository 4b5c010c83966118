"""Opacity stage at production shapes against an independent float64 numpy reference.

The GPU planes of ``k_opacity_gas`` (FUSE 0 / 1 / 2 / 3), ``k_level_sums``, ``k_compute_opacity`` and
``k_compute_opacity_facets``, reached through the launch code of picaso_amd/optics.py, against
[host tables -> oracle/optics_oracle.py table queries (interp_molecular, nearest_molecular,
continuum_nearest, pre_mix_ck, continuum_ck) -> gas_sums -> compute_opacity], the chain the CPU tests
pin to tests/golden/optics.npz and ck.npz.  Bracketing (P,T) rows of the linear query come from
``RetrieveOpacities.find_needed_pts`` (host code pinned by the same fixtures); every per-(layer,
wavelength) number of the reference is the oracle's.  All inputs are generated here (synthetic tables,
profiles, cloud slabs, a premixed ln-kappa table with 8 Gauss points).

Shapes: layer counts hit every tail of the 6- and 10-layer tiles and of k_level_sums' 8-layer loop;
wavelength counts sit on both sides of 8 column groups (the XCD-ordered block mapping) up to 1e5.  3-D:
facet counts whose 1024-column blocks straddle wavelengths, 64 facets, and the chunked facet-major
launches (12 molecules: chunks of 56 + 8 facets; the correlated-k route and the facet-fastest route with cloud
tables, which no affordable shape chunks, under a table budget cut down to five facets' worth).

Tolerances, elementwise with the NaN pattern exact: TAUGAS / TAURAY / species planes 1e-13, the 13
planes 1e-12; ``tau`` is np.cumsum of ``dtau`` and regridded cloud tables are numpy.interp's, bit for
bit.  Largest relative errors observed on the MI355X: TAUGAS 3.2e-14 (correlated-k 2.9e-14), TAURAY
4.3e-16, species planes 3.7e-14, the 13 planes 3.2e-14 (1-D), 3.3e-14 (3-D and chunked), 2.9e-14
(correlated-k); a run with -s prints them per path.  Every case also asserts
that the reference of the neighbouring layer / wavelength / facet (or of the other chunk's facets) is
far outside the tolerance, so a misplaced read cannot pass."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_optics import NAMES, pollack_table  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

TOL_GAS, TOL_PLANES = 1e-13, 1e-12
MISPLACED = 1e-8             # a misplaced read must be off by at least this much (1e4 x the loosest tolerance)
TEMPS, PRESS = [100.0, 300.0, 700.0, 1500.0, 3000.0], [1e-6, 1e-4, 1e-2, 1.0, 100.0, 500.0]
SHAPES = [(1, 1), (5, 255), (7, 1793), (11, 2048), (13, 2049), (17, 4097), (59, 12501), (90, 100000)]
OBSERVED = {}                # path -> largest relative error seen (printed with -s)


def _rel(got, want, tol, what):
    """elementwise relative error (absolute where the reference is 0); NaN patterns must match"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    den = np.where(np.abs(want) > 0, np.abs(want), 1.0)
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.where(np.isnan(want), 0.0, np.abs(got - want) / den))) if got.size else 0.0
    key = what[0] if isinstance(what, tuple) else what
    OBSERVED[key] = max(err, OBSERVED.get(key, 0.0))
    assert err <= tol, (what, err)
    return err


def _far(got, wrong, what, axis=0, frac=1.0):
    """slice by slice along ``axis``, the result is far (> MISPLACED) from the reference of the wrong place; with
    ``frac`` < 1 for that share of the slices (neighbouring wavelengths of a smooth table can nearly coincide)"""
    den = np.where(np.abs(wrong) > 0, np.abs(wrong), 1.0)
    other = tuple(i for i in range(got.ndim) if i != axis)
    worst = np.nanmax(np.abs(got - wrong) / den, axis=other)
    assert np.mean(worst > MISPLACED) >= frac, (what, axis, float(np.min(worst)))


def _misplaced(got, want, axis, what):
    """a read one step off along ``axis`` (layer, wavelength, facet) would fail: the reference one step along is far
    from the result (wavelengths: 99 % of them)"""
    n = got.shape[axis]
    if n < 2:
        return
    a, b = np.take(got, range(1, n), axis=axis), np.take(want, range(n - 1), axis=axis)
    _far(a, b, what, axis, frac=1.0 if axis != 1 else 0.99)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest relative errors: " + ", ".join("%s %.2e" % kv for kv in sorted(OBSERVED.items())))


# ------------------------------------------------------------------------------------------------ reference
def _mols(n):
    return tuple(["H2O", "CH4", "CO", "CO2", "NH3", "Na", "K", "TiO", "VO", "FeH", "H2S", "PH3"][:n])


class Tables:
    """the synthetic tables: the opacity object on the device and the host arrays the reference reads"""

    def __init__(self, nwno, qm="linear", mols=("H2O", "CH4"), wno=None):
        from picaso_amd import optics as px
        from picaso_amd import synthetic as syn
        self.raw = syn.opacity_tables(nwno, mols=mols, wno=wno)
        self.opa = px.RetrieveOpacities(query_method=qm, **self.raw)
        self.qm, self.mols = qm, mols
        self.pt = sorted(self.raw["pt_pairs"])
        self.rows = {m: np.stack([self.raw["molecular"][m][pid] for pid, _, _ in self.pt]) for m in mols}
        self.cia_t = sorted(self.raw["cia_temps"])
        self.cia = {k: np.stack([v[t] for t in self.cia_t]) for k, v in self.raw["continuum"].items()}


def _layers(atm):
    """per-layer inputs of the sums, as ATMSETUP gives them"""
    mix = atm.layer["mixingratios"]
    x = {m: np.asarray(mix[m].values if hasattr(mix[m], "values") else mix[m], dtype=float) for m in mix}
    pconv = atm.c.pconv
    return dict(mix=x, tlevel=np.asarray(atm.level["temperature"], dtype=float),
                plevel=np.asarray(atm.level["pressure"], dtype=float) / pconv,
                tlayer=np.asarray(atm.layer["temperature"], dtype=float),
                player=np.asarray(atm.layer["pressure"], dtype=float) / pconv,
                colden=np.asarray(atm.layer["colden"], dtype=float), mmw=np.asarray(atm.layer["mmw"], dtype=float),
                gravity=float(atm.planet.gravity), rgas=atm.c.rgas)


def reference_gas(atm, T, ck=None):
    """(taugas, tauray, terms) of one 1-D atmosphere: the oracle's table queries and sums"""
    from oracle import optics_oracle as oo
    L = _layers(atm)
    coef = oo.coef1(L["tlevel"], L["plevel"], L["gravity"], L["mmw"], rgas=L["rgas"])
    pairs = [(a, b) for a, b in atm.continuum_molecules]
    ray = [(m, T.raw["rayleigh_opa"][m]) for m in atm.rayleigh_molecules if m in T.raw["rayleigh_opa"]]
    if ck is not None:
        cont = [((a, b), oo.continuum_ck(L["tlayer"], ck["cia_t"], ck["cia"][a + b])) for a, b in pairs]
        mol = oo.pre_mix_ck(L["player"], L["tlayer"], np.array(PRESS), np.array(TEMPS), ck["nc_p"], ck["ln_kappa"])
        return oo.gas_sums(L["colden"], L["mmw"], L["mix"], coef, continuum=cont, rayleigh=ray, premixed=mol)
    cont = [((a, b), oo.continuum_nearest(L["tlayer"], T.cia_t, T.cia[a + b])) for a, b in pairs]
    mols = [m for m in atm.molecules if m in T.mols]
    if T.qm == "linear":
        t_i, p_i, i_ll, i_hl, i_lh, i_hh = T.opa.find_needed_pts(L["tlayer"], L["player"])
        mol = [(m, oo.interp_molecular(T.rows[m], t_i[:, 0], p_i[:, 0], i_ll, i_hl, i_hh, i_lh)) for m in mols]
    else:
        mol = [(m, oo.nearest_molecular(T.rows[m], T.pt, L["player"], L["tlayer"])[0]) for m in mols]
    return oo.gas_sums(L["colden"], L["mmw"], L["mix"], coef, continuum=cont, molecular=mol, rayleigh=ray)


def reference_planes(tg, tr, cld=None, rf=0.99999):
    from oracle import optics_oracle as oo
    z = np.zeros(tr.shape)
    c = (z, z, z) if cld is None else (cld["opd"], cld["w0"], cld["g0"])
    if tg.ndim == 3:
        c = tuple(x[:, :, None] for x in c)
        tr = tr[:, :, None]
    out = oo.compute_opacity(tg, tr, *c, rf, stream=2, delta_eddington=True)
    # (correlated-k: the planes of the cloud / Rayleigh terms alone repeat over the Gauss points, as the reference's)
    return {k: np.broadcast_to(v, (v.shape[0],) + tg.shape[1:]) for k, v in zip(NAMES, out)}


def _profile(nlevel, mols, shift=0.0):
    """level profile whose neighbouring layers bracket different table rows (non-monotonic temperature)"""
    p = np.logspace(-6.0, 2.5, nlevel)
    x = np.linspace(0.0, 1.0, nlevel)
    t = 120.0 + 1400.0 * x ** 1.5 * (1.0 + 0.35 * np.sin(1.7 * np.arange(nlevel) + shift))
    prof = {"pressure": p, "temperature": t, "H2": np.full(nlevel, 0.84), "He": np.full(nlevel, 0.155)}
    for i, m in enumerate(mols):
        prof[m] = np.full(nlevel, 1e-3 / (1.5 ** i)) * (1.0 + 0.3 * x)
    return prof


def _atmosphere(T, nlayer, shift=0.0):
    from picaso_amd import justdoit as jdi
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=2500.0)
    case.atmosphere(df=_profile(nlayer + 1, T.mols, shift))
    case.approx(raman="none")
    atm = jdi._setup_atmosphere(case.inputs, T.opa, T.opa.wno)
    return atm


def _cloud_planes(nlayer, nwno):
    from picaso_amd import synthetic as syn
    return syn.cloud_slab(nlayer, nwno, top=0.3, thickness=max(1, nlayer // 2))


def _cloud_tables(nlayer, nin=196):
    """compact tables on a grid of their own that the opacity grid overhangs at both ends"""
    xp = np.linspace(4000.0, 25000.0, nin)
    rng = np.random.default_rng(nlayer)
    lay = (np.arange(nlayer) >= nlayer // 3)[:, None]
    return xp, {"opd": lay * rng.uniform(0.05, 2.0, (nlayer, nin)), "w0": lay * rng.uniform(0.5, 0.999, (nlayer, nin)),
                "g0": lay * rng.uniform(0.0, 0.9, (nlayer, nin))}


def _host(d):
    return {k: v.to_host() for k, v in d.items() if not k.startswith("_")}


def _check_planes(got, want, what, names=None):
    for k in (names or NAMES):
        _rel(got[k], want[k], TOL_PLANES, (what + "/planes", k))
    for lvl, lay in (("tau", "dtau"), ("tau_og", "dtau_og")):
        if lvl in got:
            g = got[lvl]
            assert np.all(g[0] == 0) and np.array_equal(g[1:], np.cumsum(got[lay], axis=0)), (what, lvl)


# ------------------------------------------------------------------------------------------------ 1-D
@pytest.mark.parametrize("qm", ["linear", "nearest"])
@pytest.mark.parametrize("nlayer,nwno", SHAPES)
def test_1d_opacity_stage_against_numpy(nlayer, nwno, qm, monkeypatch):
    """Every 1-D form of the opacity stage at one shape: the default fused launch with cloud planes and with cloud
    tables on their own grid (FUSE 1), the cloud-free lean launch (FUSE 2), the two launches with TAUGAS / TAURAY read
    back (full_output: FUSE 0 + k_compute_opacity) and the species planes of return_mode (FUSE 3)."""
    from picaso_amd import optics as px
    from picaso_amd.atmsetup import CloudTables
    T = Tables(nwno, qm)
    atm = _atmosphere(T, nlayer)
    opa = T.opa
    opa.get_opacities(atm)
    tg, tr, terms = reference_gas(atm, T)
    # (1) fused, cloud planes on the opacity grid
    cld = _cloud_planes(nlayer, nwno)
    atm.layer["cloud"], atm.cloud_free = cld, False
    want = reference_planes(tg, tr, cld)
    got = _host(px.compute_opacity_resident(atm, opa, raman=2))
    _check_planes(got, want, "1d/fused")
    assert np.array_equal(got["cosb_og"], cld["g0"])
    _misplaced(got["dtau_og"], want["dtau_og"], 0, "1d/fused")
    _misplaced(got["dtau_og"], want["dtau_og"], 1, "1d/fused")
    # (2) the same through the two launches, TAUGAS / TAURAY themselves
    monkeypatch.setenv("PICASO_AMD_UNFUSED_OPACITY", "1")
    got2 = _host(px.compute_opacity_resident(atm, opa, raman=2, full_output=True))
    monkeypatch.delenv("PICASO_AMD_UNFUSED_OPACITY")
    _rel(atm.taugas[:, :, 0], tg, TOL_GAS, "1d/taugas")
    _rel(atm.tauray[:, :, 0], tr, TOL_GAS, "1d/tauray")
    _misplaced(atm.taugas[:, :, 0], tg, 0, "1d/taugas")
    _misplaced(atm.taugas[:, :, 0], tg, 1, "1d/taugas")
    _check_planes(got2, want, "1d/unfused")
    # (3) species planes: each against its own term of the reference sum
    sp = px.compute_opacity(atm, opa, return_mode=True)
    assert list(sp) == list(terms) + ["cloud"]
    for k, v in terms.items():
        _rel(sp[k], v, TOL_GAS, ("1d/species", k))
        _misplaced(sp[k], v, 0, ("1d/species", k))
    assert np.array_equal(sp["cloud"], cld["opd"])
    # (4) cloud tables on their own grid, interpolated inside the fused launch
    xp, compact = _cloud_tables(nlayer)
    atm.layer["cloud"] = CloudTables(compact, xp, opa.wno)
    cplanes = {k: np.stack([np.interp(opa.wno, xp, row) for row in compact[k]]) for k in compact}
    got = _host(px.compute_opacity_resident(atm, opa, raman=2))
    _check_planes(got, reference_planes(tg, tr, cplanes), "1d/fused-tables")
    assert np.array_equal(got["cosb_og"], cplanes["g0"])                   # numpy.interp's bits
    # (5) cloud-free, the lean form
    atm.layer["cloud"], atm.cloud_free = {k: np.zeros((nlayer, nwno)) for k in ("opd", "w0", "g0")}, True
    lean = ("dtau", "w0", "w0_no_raman")
    got = _host(px.compute_opacity_resident(atm, opa, raman=2, want=set(lean)))
    assert sorted(got) == sorted(lean)
    want = reference_planes(tg, tr)
    _check_planes(got, want, "1d/lean", names=lean)
    _misplaced(got["dtau"], want["dtau"], 0, "1d/lean")


# ------------------------------------------------------------------------------------------------ correlated-k
def _ck_tables(nwno, ngauss=8):
    from picaso_amd import optics as px
    from picaso_amd import synthetic as syn
    raw = syn.opacity_tables(nwno, mols=())
    wno = raw["wno"]
    nc_p = np.full(len(TEMPS), len(PRESS))
    lp, lt = np.log10(PRESS)[:, None, None, None], np.log10(np.array(TEMPS) / 300.0)[None, :, None, None]
    g = np.linspace(0.0, 1.0, ngauss)[None, None, None, :]
    w = (wno / 2500.0)[None, None, :, None]
    ln_kappa = np.log(1e-24) + 4.0 * np.sin(w) + 0.9 * lp + 1.8 * lt + 3.0 * g * (1.0 + 0.3 * np.cos(w + lp))
    gw = np.full(ngauss, 1.0 / ngauss)
    pressures = np.concatenate([PRESS for _ in TEMPS])
    temps = np.concatenate([[t] * len(PRESS) for t in TEMPS])
    opa = px.RetrieveCKs(wno, gw, pressures, temps, nc_p, ln_kappa, continuum=raw["continuum"],
                         cia_temps=raw["cia_temps"], rayleigh_opa=raw["rayleigh_opa"])
    cia_t = sorted(raw["cia_temps"])
    ck = dict(ln_kappa=ln_kappa, nc_p=nc_p, cia_t=cia_t,
              cia={k: np.stack([v[t] for t in cia_t]) for k, v in raw["continuum"].items()})
    T = Tables.__new__(Tables)
    T.raw, T.opa, T.qm, T.mols = raw, opa, "premixed", ()
    return T, ck


@pytest.mark.parametrize("nlayer,nwno", [(7, 257), (90, 257), (7, 12501), (90, 12501)])
def test_ck_opacity_stage_against_numpy(nlayer, nwno):
    """Premixed correlated-k with 8 Gauss points: 257 wavelengths are 2056 columns, 9 column groups (one in the tail
    of the XCD-ordered mapping).  TAUGAS (nlayer, nwno, 8) / TAURAY read back, the 13 planes with a cloud slab."""
    from picaso_amd import optics as px
    T, ck = _ck_tables(nwno)
    atm = _atmosphere(T, nlayer)
    T.opa.get_opacities(atm)
    tg, tr, _ = reference_gas(atm, T, ck=ck)
    assert tg.shape == (nlayer, nwno, 8)
    cld = _cloud_planes(nlayer, nwno)
    atm.layer["cloud"], atm.cloud_free = cld, False
    got = _host(px.compute_opacity_resident(atm, T.opa, ngauss=8, raman=2, full_output=True))
    _rel(atm.taugas, tg, TOL_GAS, "ck/taugas")
    _rel(atm.tauray[:, :, 0], tr, TOL_GAS, "ck/tauray")
    for ax in (0, 1, 2):
        _misplaced(atm.taugas, tg, ax, "ck/taugas")
    _check_planes(got, reference_planes(tg, tr, cld), "ck")


# ------------------------------------------------------------------------------------------------ 3-D
def _facets(T, nlayer, ng, nt, amplitude=0.1):
    """facet-form atmosphere of per-facet temperature profiles and the 1-D atmosphere of every facet"""
    from picaso_amd import justdoit as jdi
    from picaso_amd import synthetic as syn
    from picaso_amd.spectrum import setup_facets_3d
    case = jdi.inputs()
    case.phase_angle(0, num_gangle=ng, num_tangle=nt)
    case.gravity(gravity=2500.0)
    case.atmosphere_3d(syn.facet_profiles(nlayer + 1, ng, nt, mols=T.mols, amplitude=amplitude))
    case.approx(raman="none")
    atm_f = setup_facets_3d(case.inputs, T.opa, T.opa.wno, ng, nt)[0]
    prof3 = case.inputs["atmosphere"]["profile_3d"]
    ones = [jdi._setup_atmosphere(case.inputs, T.opa, T.opa.wno,
                                  {k: (v if np.ndim(v) == 1 else v[:, g, t]) for k, v in prof3.items()}, None)
            for g in range(ng) for t in range(nt)]
    return atm_f, ones


def _facet_refs(T, ones, ck=None):
    return [reference_gas(a, T, ck=ck)[:2] for a in ones]


@pytest.mark.parametrize("ng,nt", [(3, 2), (4, 3), (5, 5), (8, 8)])
def test_3d_opacity_facets_against_numpy(ng, nt, monkeypatch):
    """compute_opacity_facets (batched gas stage + the LDS-staged facet kernel, and the direct kernel under
    PICASO_AMD_MIX_DIRECT) and compute_opacity_facet_major (cloud-free, and with cloud tables on their own grid) on
    per-facet temperature profiles, 3001 wavelengths: each facet's planes against the 1-D reference of its profile."""
    from picaso_amd import optics as px
    nwno, nlayer, nfac = 3001, (90 if ng * nt == 64 else 23), ng * nt
    T = Tables(nwno, "linear")
    atm_f, ones = _facets(T, nlayer, ng, nt)
    refs = _facet_refs(T, ones)
    cld = _cloud_planes(nlayer, nwno)
    want = [reference_planes(tg, tr, cld) for tg, tr in refs]
    for direct in (False, True):
        if direct:
            monkeypatch.setenv("PICASO_AMD_MIX_DIRECT", "1")
        got = _host(px.compute_opacity_facets(atm_f, T.opa, ng, nt, raman=2, clouds_3d=cld))
        monkeypatch.delenv("PICASO_AMD_MIX_DIRECT", raising=False)
        what = "3d/facets" + ("-direct" if direct else "")
        for f in range(nfac):
            one = {k: v[:, :, f // nt, f % nt] for k, v in got.items()}
            _check_planes(one, want[f], what)
        stack = np.stack([got["dtau"][:, :, f // nt, f % nt] for f in range(nfac)])
        _misplaced(stack, np.stack([w["dtau"] for w in want]), 0, what)
    # facet-major, cloud-free: the lean planes
    lean = ("dtau", "w0", "w0_no_raman")
    got = _host(px.compute_opacity_facet_major(atm_f, T.opa, ng, nt, raman=2, want=lean))
    clear = [reference_planes(tg, tr) for tg, tr in refs]
    for f in range(nfac):
        _check_planes({k: got[k][f] for k in lean}, clear[f], "3d/facet-major", names=lean)
    _misplaced(got["dtau"], np.stack([w["dtau"] for w in clear]), 0, "3d/facet-major")
    # facet-major with cloud tables on their own grid, interpolated inside the fused launch
    xp, compact = _cloud_tables(nlayer)
    cld3 = dict(compact, wavenumber=xp)
    tabs = px._facet_major_cloud_tables(cld3, nlayer, nfac, T.opa.ctx)
    layer_planes = tuple(k for k in NAMES if k not in ("tau", "tau_og"))
    got = _host(px.compute_opacity_facet_major(atm_f, T.opa, ng, nt, raman=2, want=layer_planes, cloud_tables=tabs))
    cplanes = {k: np.stack([np.interp(T.opa.wno, xp, row) for row in compact[k]]) for k in compact}
    for f in range(nfac):
        w = reference_planes(*refs[f], cplanes)
        _check_planes({k: got[k][f] for k in layer_planes}, w, "3d/facet-major-tables", names=layer_planes)
        assert np.array_equal(got["cosb_og"][f], cplanes["g0"])


def test_3d_facet_major_ck_against_numpy():
    """compute_opacity_facet_major_ck: 12 facets x 23 layers x 257 wavelengths x 8 Gauss points, per-facet
    temperatures, a cloud slab; every facet's 13 planes against its 1-D correlated-k reference."""
    from picaso_amd import optics as px
    ng, nt, nlayer = 4, 3, 23
    T, ck = _ck_tables(257)
    atm_f, ones = _facets(T, nlayer, ng, nt)
    cld = _cloud_planes(nlayer, 257)
    got = _host(px.compute_opacity_facet_major_ck(atm_f, T.opa, ng, nt, raman=2, clouds_3d=cld))
    want = [reference_planes(tg, tr, cld) for tg, tr in _facet_refs(T, ones, ck=ck)]
    for f in range(ng * nt):
        _check_planes({k: got[k][f] for k in NAMES}, want[f], "3d/facet-major-ck")
    _misplaced(got["dtau"], np.stack([w["dtau"] for w in want]), 0, "3d/facet-major-ck")


# ------------------------------------------------------------------------------------------------ chunked launches
@pytest.fixture(scope="module")
def chunked():
    """64 facets x 90 layers x 12 molecules on 3001 wavelengths: the per-layer tables need two launches (56 + 8)"""
    T = Tables(3001, "linear", mols=_mols(12))
    atm_f, ones = _facets(T, 90, 8, 8, amplitude=0.25)
    return T, atm_f, ones, _facet_refs(T, ones)


def _count_gas_calls(monkeypatch, tables=None):
    from picaso_amd import optics as px
    calls = []
    real = px._gas_call

    def spy(*a, **k):
        calls.append(a[1])                 # nlayer of the launch
        if tables is not None:
            tables.append(k)               # ... and its tables
        return real(*a, **k)
    monkeypatch.setattr(px, "_gas_call", spy)
    return calls


def test_chunked_gas_stage_facets(chunked, monkeypatch):
    """gas_stage_facets in two launches: TAUGAS / TAURAY of every facet against its reference; the second chunk's
    facets are far from the first chunk's references."""
    from picaso_amd import optics as px
    from picaso_amd.device import DeviceArray
    T, atm_f, ones, refs = chunked
    calls = _count_gas_calls(monkeypatch)
    tg3, tr3 = DeviceArray((64, 90, 3001), T.opa.ctx), DeviceArray((64, 90, 3001), T.opa.ctx)
    px.gas_stage_facets(atm_f, T.opa, 64, tg3, tr3)
    assert calls == [56 * 90, 8 * 90]
    tg, tr = tg3.to_host(), tr3.to_host()
    for f in range(64):
        _rel(tg[f], refs[f][0], TOL_GAS, "chunked/taugas")
        _rel(tr[f], refs[f][1], TOL_GAS, "chunked/tauray")
    _far(tg[56:], np.stack([r[0] for r in refs[:8]]), "chunked/taugas")


@pytest.mark.parametrize("raman", ["none", "pollack", "oklopcic", "pollack-host-plane"])
def test_chunked_facet_major_raman(chunked, raman, monkeypatch, pollack_table):  # noqa: F811
    """compute_opacity_facet_major in two launches with each Raman form: every facet's dtau / w0 / w0_no_raman against
    the reference with that facet's Raman factor (Oklopcic: optics.compute_raman of the facet's layer temperatures;
    Pollack: the table row, also as the host-made plane of PICASO_AMD_RAMAN_PLANES).  Each chunk must read the Raman
    rows of its own facets: for Oklopcic, w0 of facets 56.. is far from the reference built on facets 0..7's factor."""
    from picaso_amd import optics as px
    T, atm_f, ones, refs = chunked
    opa = T.opa
    wno = opa.wno
    code = {"none": 2, "pollack": 1, "oklopcic": 0, "pollack-host-plane": 1}[raman]
    if raman == "pollack-host-plane":
        monkeypatch.setenv("PICASO_AMD_RAMAN_PLANES", "1")
    if code == 0:
        g = np.load(os.path.join(GOLDEN, "optics.npz"))
        db = {"c": g["in/raman_c"], "ji": g["in/raman_ji"], "deltanu": g["in/raman_deltanu"]}
        opa.raman_db = db
        opa.raman_stellar_shifts = 1.0 + 0.3 * np.sin(np.outer(wno / 900.0, 1.0 + np.arange(db["c"].size) / 7.0))
    calls = _count_gas_calls(monkeypatch)
    lean = ("dtau", "w0", "w0_no_raman")
    got = _host(px.compute_opacity_facet_major(atm_f, opa, 8, 8, raman=code, want=lean))
    assert calls == [56 * 90, 8 * 90]
    rfs = []
    for f in range(64):
        if code == 0:
            tl = np.asarray(ones[f].layer["temperature"], dtype=float)
            rf = np.minimum(px.compute_raman(opa.nwno, 90, wno, opa.raman_stellar_shifts, tl, db["c"], db["ji"],
                                             db["deltanu"]), 0.99999)
        elif code == 1:
            rf = np.minimum(px.raman_pollack(90, 1e4 / wno), 0.99999)
        else:
            rf = 0.99999
        rfs.append(rf)
        want = reference_planes(*refs[f], rf=rf)
        _check_planes({k: got[k][f] for k in lean}, want, "chunked/facet-major-" + raman, names=lean)
    if code == 0:
        # the reference of facets 56..63 built on facets 0..7's Raman factor is far from the result
        wrong = np.stack([reference_planes(*refs[56 + f], rf=rfs[f])["w0"] for f in range(8)])
        _far(got["w0"][56:], wrong, "chunked/raman")
    _far(got["dtau"][56:], np.stack([reference_planes(*r)["dtau"] for r in refs[:8]]), "chunked/facet-major")


def _budget_of_facets(monkeypatch, nfacets, nlayer, tables):
    """the table budget of one gas launch cut down to ``nfacets`` facets' worth of a recorded launch's tables"""
    from picaso_amd import optics as px
    counts = [len(tables[k]) for k in ("mol_tabs", "cont_tabs", "ray_tabs")]
    monkeypatch.setattr(px, "GAS_TABLE_BUDGET", nfacets * px.gas_table_bytes(*counts, nlayer, tables["cont_wts"]))


def test_chunked_facet_major_ck(monkeypatch):
    """compute_opacity_facet_major_ck in three launches (5 + 5 + 2 of 12 facets; no affordable shape overflows the real
    budget): the 13 planes are those of the single launch bit for bit and every facet's are its 1-D correlated-k
    reference's; the last chunk's facets are far from the first facets' references."""
    from picaso_amd import optics as px
    ng, nt, nlayer = 4, 3, 23
    T, ck = _ck_tables(257)
    atm_f, ones = _facets(T, nlayer, ng, nt)
    cld = _cloud_planes(nlayer, 257)
    tables = []
    calls = _count_gas_calls(monkeypatch, tables)
    whole = _host(px.compute_opacity_facet_major_ck(atm_f, T.opa, ng, nt, raman=2, clouds_3d=cld))
    assert calls == [12 * 23]
    _budget_of_facets(monkeypatch, 5, nlayer, tables[0])
    del calls[:]
    got = _host(px.compute_opacity_facet_major_ck(atm_f, T.opa, ng, nt, raman=2, clouds_3d=cld))
    assert calls == [5 * 23, 5 * 23, 2 * 23]
    assert sorted(got) == sorted(NAMES)
    for k in NAMES:
        assert np.array_equal(got[k], whole[k]), k
    want = [reference_planes(tg, tr, cld) for tg, tr in _facet_refs(T, ones, ck=ck)]
    for f in range(ng * nt):
        _check_planes({k: got[k][f] for k in NAMES}, want[f], "chunked/facet-major-ck")
    _far(got["dtau"][10:], np.stack([w["dtau"] for w in want[:2]]), "chunked/facet-major-ck")


def test_chunked_facets_cloud_tables(monkeypatch):
    """compute_opacity_facets with cloud tables on their own grid, its gas stage in two launches (5 + 1 of 6 facets):
    the planes of the single launch bit for bit."""
    from picaso_amd import optics as px
    ng, nt, nlayer = 3, 2, 23
    T = Tables(3001, "linear")
    atm_f, _ = _facets(T, nlayer, ng, nt)
    xp, compact = _cloud_tables(nlayer)
    cld3 = dict(compact, wavenumber=xp)
    tables = []
    calls = _count_gas_calls(monkeypatch, tables)
    whole = _host(px.compute_opacity_facets(atm_f, T.opa, ng, nt, raman=2, clouds_3d=cld3))
    assert calls == [6 * 23]
    _budget_of_facets(monkeypatch, 5, nlayer, tables[0])
    del calls[:]
    got = _host(px.compute_opacity_facets(atm_f, T.opa, ng, nt, raman=2, clouds_3d=cld3))
    assert calls == [5 * 23, 1 * 23]
    assert sorted(got) == sorted(NAMES)
    for k in NAMES:
        assert np.array_equal(got[k], whole[k]), k
