"""The tall-atmosphere front end of the 3-D opacity stage (picaso_amd/optics.py), host side: the byte count that cuts
the facets into gas launches against the packing of ``gas_launch`` (csrc/optics.hip), the launches the generator
yields, the facet-major flattening and the normalisation of a cloud dictionary's wavenumber grid."""
import itertools
import types

import numpy as np
import pytest

from picaso_amd import optics as px

SLOT_BYTES = 4 << 20                      # picaso_ctx::SLOT_BYTES (csrc/common.hpp)
COUNTS = list(itertools.product(range(15), range(5), range(7), (None, True)))      # nmol, ncont, nray, cont_wts


def _packed_per_layer(nmol, ncont, nray, cont_wts):
    """bytes per layer gas_launch packs: int rows (4 per molecule, crow per pair), weights, coefficients"""
    crow = 2 if cont_wts is not None else 1
    return nmol * (16 + 32 + 8) + ncont * (4 * crow + 16 * (crow - 1) + 8) + nray * 8


def test_gas_table_bytes_against_gas_launch_packing():
    for nmol, ncont, nray, cont_wts in COUNTS:
        packed = _packed_per_layer(nmol, ncont, nray, cont_wts)
        for nlayer in (1, 23, 90, 5760):
            got = px.gas_table_bytes(nmol, ncont, nray, nlayer, cont_wts)
            assert got >= packed * nlayer
            assert got == (packed + 8) * nlayer, (nmol, ncont, nray, cont_wts, nlayer)
    assert px.gas_table_bytes(3, 2, 1, 7) == px.gas_table_bytes(3, 2, 1, 7, None)
    # a launch that fills the budget still fits the slot with its table pointers, alignment padding and spare bytes
    assert px.GAS_TABLE_BUDGET == 3600 * 1024
    assert px.GAS_TABLE_BUDGET + 8 * (14 + 4 + 6) + 64 + 3 * 8 <= SLOT_BYTES


def _fake_opacity(nmol, ncont, nray, ntot, ck):
    """what _gas_tables reads of an opacity object and its tall plan, with every per-layer entry = its layer index"""
    mols, pairs, rays = (["m%d" % i for i in range(n)] for n in (nmol, ncont, nray))
    lay = np.arange(ntot)
    plan = dict(molecules=["premixed"] if ck else mols, cia_pairs=pairs,
                rows=np.broadcast_to(lay[None, :, None], (1 if ck else nmol, ntot, 4)).astype(np.int32),
                wts=np.broadcast_to(lay[None, :, None], (1 if ck else nmol, ntot, 4)).astype(float),
                cia_rows=np.broadcast_to(lay[:, None], (ntot, 2)).astype(np.int32) if ck else lay.astype(np.int32))
    if ck:
        plan.update(premixed=True, cia_wts=np.broadcast_to(lay[:, None], (ntot, 2)).astype(float))
    tabs = {"m%d" % i: object() for i in range(15)}
    opa = types.SimpleNamespace(_plan=plan, _cia=tabs, _ray=tabs, _mol_raw=tabs, _mol_log=tabs, _kappa=object(),
                                query_method="premixed" if ck else "nearest")
    fac = lambda n: np.broadcast_to(lay[None].astype(float), (n, ntot))           # noqa: E731
    return opa, (fac(1 if ck else nmol), fac(ncont), rays, fac(nray))


def _check_launches(launches, nlayer, nfac, fchunk, nmol, ncont, nray, ck):
    assert [f0 for f0, _, _, _ in launches] == list(range(0, nfac, fchunk))           # tiles 0..nfac: no gap, no overlap
    assert [f1 for _, f1, _, _ in launches] == [min(nfac, f0 + fchunk) for f0 in range(0, nfac, fchunk)]
    for f0, f1, sl, kw in launches:
        assert (sl.start, sl.stop, sl.step) == (f0 * nlayer, f1 * nlayer, None)
        want = np.arange(f0 * nlayer, f1 * nlayer)
        assert (len(kw["mol_tabs"]), len(kw["cont_tabs"]), len(kw["ray_tabs"])) == (nmol, ncont, nray)
        assert kw["mol_mode"] == (2 if ck else 0)
        per_layer = [kw["mol_rows"][:, :, 0], kw["mol_wts"][:, :, 0], kw["mol_fac"]] if nmol else []
        per_layer += [kw["cont_rows"].reshape(ncont, len(want), -1)[:, :, 0], kw["cont_fac"]] if ncont else []
        per_layer += [kw["cont_wts"][:, :, 0]] if ncont and ck else []
        per_layer += [kw["ray_fac"]] if nray else []
        assert (kw["cont_wts"] is not None) == bool(ncont and ck)
        for a in per_layer:                                    # every table holds this launch's layers, in order
            assert np.array_equal(a, np.broadcast_to(want, a.shape))


@pytest.mark.parametrize("nlayer", [1, 23, 90])
@pytest.mark.parametrize("nfac", [1, 6, 64])
def test_tall_gas_launches_tile_the_facets(nlayer, nfac):
    for nmol, ncont, nray, cont_wts in COUNTS:
        ck = cont_wts is not None
        if ck and nmol != 1:                                   # a premixed plan has ONE molecular table
            continue
        opa, factors = _fake_opacity(nmol, ncont, nray, nfac * nlayer, ck)
        per_layer = _packed_per_layer(nmol, ncont, nray, cont_wts) + 8
        fchunk = max(1, (3600 * 1024) // (per_layer * nlayer))
        launches = list(px._tall_gas_launches(opa, factors, nlayer, nfac))
        _check_launches(launches, nlayer, nfac, fchunk, nmol, ncont, nray, ck)


@pytest.mark.parametrize("ck", [False, True])
@pytest.mark.parametrize("facets_worth", [0, 1, 5, 7])
def test_tall_gas_launches_follow_the_budget(ck, facets_worth, monkeypatch):
    """the budget is read when the launches are cut: 12 facets in chunks of 5 + 5 + 2, of 7 + 5, and one by one when not
    even one facet fits"""
    nlayer, nfac, (nmol, ncont, nray) = 23, 12, ((1, 3, 2) if ck else (4, 3, 2))
    opa, factors = _fake_opacity(nmol, ncont, nray, nfac * nlayer, ck)
    monkeypatch.setattr(px, "GAS_TABLE_BUDGET",
                        facets_worth * px.gas_table_bytes(nmol, ncont, nray, nlayer, True if ck else None))
    launches = list(px._tall_gas_launches(opa, factors, nlayer, nfac))
    _check_launches(launches, nlayer, nfac, max(1, facets_worth), nmol, ncont, nray, ck)
    assert [(f1 - f0) * nlayer for f0, f1, _, _ in launches] == {0: [23] * 12, 1: [23] * 12, 5: [115, 115, 46],
                                                                 7: [161, 115]}[facets_worth]


def test_tall_atmosphere_is_facet_major():
    nlayer, nfac = 2, 4                                        # 3 levels, 2 x 2 facets
    temp = 100.0 * np.arange(1, nlayer + 1)[:, None] + np.arange(nfac)[None, :]       # (nlayer, nfacets)
    pres = np.array([[1e3], [1e5]])                                                     # shared: (nlayer, 1)
    atm_f = types.SimpleNamespace(
        c=types.SimpleNamespace(nlayer=nlayer, pconv=1e6),
        layer={"temperature": temp, "pressure": pres,
               "mixingratios": {"H2O": 1e-3 * (1.0 + temp), "CH4": np.array([[1e-4], [2e-4]])}},
        molecules=["H2O", "CH4"], continuum_molecules=[("H2", "H2")])
    tall = px._tall_atmosphere(atm_f, nfac)
    assert tall.c.nlayer == nfac * nlayer and tall.c.pconv == 1e6
    assert tall.molecules is atm_f.molecules and tall.continuum_molecules is atm_f.continuum_molecules
    assert set(tall.layer) == {"temperature", "pressure"}      # mixing ratios only on request
    for f in range(nfac):
        for l in range(nlayer):                                # noqa: E741
            assert tall.layer["temperature"][f * nlayer + l] == temp[l, f]
            assert tall.layer["pressure"][f * nlayer + l] == pres[l, 0]
    with_mix = px._tall_atmosphere(atm_f, nfac, mixingratios=True)
    assert np.array_equal(with_mix.layer["temperature"], tall.layer["temperature"])
    assert list(with_mix.layer["mixingratios"]) == ["H2O", "CH4"]
    for f in range(nfac):
        for l in range(nlayer):                                # noqa: E741
            assert with_mix.layer["mixingratios"]["H2O"][f * nlayer + l] == 1e-3 * (1.0 + temp[l, f])
            assert with_mix.layer["mixingratios"]["CH4"][f * nlayer + l] == [1e-4, 2e-4][l]
    for v in list(with_mix.layer["mixingratios"].values()) + [tall.layer["temperature"], tall.layer["pressure"]]:
        assert v.shape == (nfac * nlayer,) and v.dtype == np.float64 and v.flags.c_contiguous


def test_cloud_own_grid():
    wno = np.linspace(500.0, 30000.0, 11)
    tabs = {"opd": None, "w0": None, "g0": None}
    # on the opacity grid: no grid of their own
    assert px._cloud_own_grid(tabs, wno) == (None, None)
    assert px._cloud_own_grid(dict(tabs, wavenumber=None), wno) == (None, None)
    assert px._cloud_own_grid(dict(tabs, wavenumber=wno.copy()), wno) == (None, None)
    assert px._cloud_own_grid(dict(tabs, wavenumber=list(wno)), wno) == (None, None)
    # a grid of the same length that is not the opacity grid is the tables' own
    grid, order = px._cloud_own_grid(dict(tabs, wavenumber=wno + 1.0), wno)
    assert np.array_equal(grid, wno + 1.0) and order is None
    # increasing: as given, no sort
    xp = [4000, 9000, 25000]
    grid, order = px._cloud_own_grid(dict(tabs, wavenumber=xp), wno)
    assert grid.dtype == np.float64 and np.array_equal(grid, xp) and order is None
    # decreasing (with a tie): the stable sort order
    xp = np.array([25000.0, 9000.0, 9000.0, 4000.0])
    grid, order = px._cloud_own_grid(dict(tabs, wavenumber=xp), wno)
    assert np.array_equal(grid, xp)
    assert list(order) == [3, 1, 2, 0] and np.array_equal(order, np.argsort(xp, kind="stable"))
    # one wavenumber: a grid of one point (the callers take its value everywhere), nothing to sort
    for one in ([12000.0], np.float64(12000.0)):
        grid, order = px._cloud_own_grid(dict(tabs, wavenumber=one), wno)
        assert grid.shape == (1,) and grid[0] == 12000.0 and order is None
