"""inputs.clouds_4d on the GPU: the regrid launch (``picaso_gcm_facet_tables_dev``) against the host interpolation it
replaces, bit for bit, and cloudy phase curves through it against the same curves from host-built ``clouds_by_phase``.

The yardstick is the host code of the parent commit: ``justdoit._regrid_lonlat`` per phase on the map rotated as
``atmosphere_4d`` rotates it, sorted and transposed as ``clouds_3d`` does, re-stacked as
``optics._facet_major_cloud_tables`` does."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_optics import DB

pytestmark = pytest.mark.gpu

PHASES = [0.0, 0.9, 2.0]
SHIFT = np.array([0.0, 37.5, -200.0])
NLAYER = 3


def _host_tables(cloud, lon_f, lat_f, phase, shift):
    """One phase the parent's way: the dictionary ``clouds_3d`` would store for the map rotated by ``phase + shift``."""
    from picaso_amd import justdoit as jdi
    lon_rot = (np.asarray(cloud["lon"], dtype=float) + phase * 180 / np.pi + shift + 180.0) % 360.0 - 180.0
    coords = {"lon": lon_rot, "lat": np.asarray(cloud["lat"], dtype=float)}
    v = jdi._regrid_lonlat(coords, {k: np.asarray(cloud[k], dtype=float) for k in ("opd", "w0", "g0")}, lon_f, lat_f)
    order, worder = np.argsort(cloud["pressure"]), np.argsort(cloud["wno"])
    out = {k: np.ascontiguousarray(np.transpose(v[k][:, :, order][:, :, :, worder], (2, 3, 0, 1))) for k in ("opd", "w0", "g0")}
    out["wavenumber"] = np.asarray(cloud["wno"], dtype=float)[worder]
    return out


def _tall(host, nlayer, nfac):
    """The re-stack of ``optics._facet_major_cloud_tables``: (3, nfacets * nlayer, nin), opd rows, then w0, then g0."""
    nin = host["wavenumber"].size
    return np.stack([np.moveaxis(host[k].reshape(nlayer, nin, nfac), (0, 1, 2), (1, 2, 0)).reshape(nfac * nlayer, nin)
                     for k in ("opd", "w0", "g0")])


def _cloud_map(kind, nin, rng):
    lat = np.array([-60.0, -20.0, 20.0, 60.0])
    pres = np.array([1e-3, 1e-1, 3.0])
    wno = np.linspace(800.0, 9000.0, nin)
    if kind == "regional":
        lon = np.array([-40.0, -20.0, 0.0, 20.0, 40.0])
    else:
        lon = np.linspace(-180.0, 180.0, 9)
    if kind == "one_latitude":
        lat = np.array([10.0])
    shape = (lon.size, lat.size, NLAYER, nin)
    m = {"opd": rng.random(shape), "w0": 0.5 + 0.5 * rng.random(shape), "g0": rng.normal(size=shape)}
    m["opd"][:, :, 0] = 0.0                                            # nothing in the top layer
    if kind == "shuffled":          # longitudes shuffled, latitudes, pressures and wavenumbers descending
        p = rng.permutation(lon.size)
        lon = lon[p]
        lat, pres, wno = lat[::-1], pres[::-1], wno[::-1]
        m = {k: np.ascontiguousarray(v[p][:, ::-1, ::-1, ::-1]) for k, v in m.items()}
    return dict(m, lon=lon, lat=lat, pressure=pres, wno=wno)


@pytest.mark.parametrize("nin", [2, 7, 65, 196])
@pytest.mark.parametrize("kind", ["global", "regional", "shuffled", "one_latitude"])
def test_kernel_equals_host_regrid_bit_for_bit(kind, nin):
    """Every phase's rows copied back against ``_regrid_lonlat`` re-stacked: 1 x 1 and 3 x 2 facets, three phases with
    shifts that cross the seam, wavenumber counts below, across and beyond one wavefront."""
    from picaso_amd import gcm
    from picaso_amd import justdoit as jdi
    rng = np.random.default_rng(100 + nin)
    cloud = _cloud_map(kind, nin, rng)
    coords, variables = jdi._dataset_like(cloud, extra_coords=("wno",))
    cmap = gcm.GcmCloudMap.resident(coords, variables)
    geo = jdi.inputs()
    geo.phase_curve_geometry("reflected", PHASES, num_gangle=3, num_tangle=2)
    facets = {
        (1, 1): ([np.array([-171.0]), np.array([3.0]), np.array([179.5])], [np.array([85.0]), np.array([-7.0]), np.array([0.0])]),
        (3, 2): ([geo.inputs["disco"][ph]["longitude"] * 180 / np.pi for ph in PHASES],
                 [geo.inputs["disco"][ph]["latitude"] * 180 / np.pi for ph in PHASES]),
    }
    for (ng, nt), (lon_f, lat_f) in facets.items():
        tabs = gcm.facet_tables(cmap, lon_f, lat_f, [(ph * 180 / np.pi, SHIFT[i]) for i, ph in enumerate(PHASES)])
        assert len(tabs) == len(PHASES)
        for i, ph in enumerate(PHASES):
            host = _host_tables(cloud, lon_f[i], lat_f[i], ph, SHIFT[i])
            want = _tall(host, NLAYER, ng * nt)
            got = tabs[i].d_tall.to_host()
            assert got.shape == want.shape == (3, ng * nt * NLAYER, nin)
            assert np.all(np.isfinite(got)) and np.array_equal(got, want), (kind, nin, ng, nt, i)
            assert not tabs[i].materialized
            for k in ("opd", "w0", "g0"):                              # the dictionary face: what clouds_3d would have stored
                assert np.array_equal(tabs[i][k], host[k])
            assert tabs[i].materialized and np.array_equal(tabs[i]["wavenumber"], host["wavenumber"])
            assert not np.any(tabs[i]["opd"][0])


# ---- through inputs: the fixture database and profile of test_ck_optics.py::test_gpu_phase_curve_equals_single_phase_runs
NG, NT = 3, 2
LON, LAT = np.linspace(-180.0, 180.0, 9), np.array([-60.0, -20.0, 20.0, 60.0])


@pytest.fixture(scope="module")
def og():
    return np.load(os.path.join(GOLDEN, "optics.npz"))


@pytest.fixture(scope="module")
def opa():
    from picaso_amd import justdoit as jdi
    return jdi.opannection(filename_db=DB, query_method="linear")


@pytest.fixture(scope="module")
def maps(og, opa):
    """The GCM (9 x 4) with a day-night temperature contrast and the cloud map on a 7-point wavenumber grid."""
    nlevel = len(og["in/tlevel"])
    rng = np.random.default_rng(8)
    contrast = 60.0 * np.cos(np.radians(LON))[:, None, None] * np.cos(np.radians(LAT))[None, :, None]
    gcm = {"lon": LON, "lat": LAT, "pressure": og["in/plevel_bar"],
           "temperature": og["in/tlevel"][None, None, :] + contrast * np.ones((1, 1, nlevel))}
    for m in ("H2", "He", "H2O", "CH4"):
        gcm[m] = np.broadcast_to(og["in/mix/" + m], (LON.size, LAT.size, nlevel)).copy()
    p = og["in/plevel_bar"]
    shape = (LON.size, LAT.size, nlevel - 1, 7)
    cloud = {"lon": LON, "lat": LAT, "pressure": np.sqrt(p[1:] * p[:-1]),
             "wno": np.linspace(opa.wno[0] * 0.98, opa.wno[-1] * 1.01, 7),
             "opd": 0.3 * rng.random(shape) * (1.0 + np.cos(np.radians(LON)))[:, None, None, None],
             "w0": 0.6 + 0.3 * rng.random(shape), "g0": 0.7 * rng.random(shape)}
    cloud["opd"][:, :, :4] = 0.0
    return gcm, cloud


def _case(og, calc, gcm):
    from picaso_amd import justdoit as jdi
    case = jdi.inputs()
    case.gravity(gravity=float(og["in/gravity"]))
    case.approx(raman="none")
    case.phase_curve_geometry(calc, PHASES, num_gangle=NG, num_tangle=NT)
    case.atmosphere_4d(gcm, shift=SHIFT, verbose=False)
    return case


def _host_by_phase(case, cloud):
    geom, shift = case.inputs["disco"], case.inputs["shift"]
    return [_host_tables(cloud, geom[ph]["longitude"] * 180 / np.pi, geom[ph]["latitude"] * 180 / np.pi, ph, shift[i])
            for i, ph in enumerate(PHASES)]


@pytest.fixture(scope="module")
def curves(og, opa, maps):
    """Per calculation: the case after clouds_4d + phase_curve, its curve, and the curve of host-built clouds_by_phase."""
    made = {}

    def get(calc):
        if calc not in made:
            gcm, cloud = maps
            case = _case(og, calc, gcm)
            case.clouds_4d(cloud, plot=False, verbose=False, calculation=calc)
            curve = case.phase_curve(opa)
            untouched = [not t.materialized for t in case.inputs["clouds"]["profile_4d"]]
            ref = _case(og, calc, gcm)
            host = _host_by_phase(ref, cloud)
            made[calc] = (case, curve, untouched, ref.phase_curve(opa, clouds_by_phase=host), host)
        return made[calc]
    return get


@pytest.mark.parametrize("calc", ["reflected", "thermal"])
def test_cloud_map_of_temperatures_lands_on_the_profiles(og, maps, calc):
    """Same rotation, same facets: a cloud map whose ``opd`` is the temperature map gives the temperatures
    ``atmosphere_4d`` stored (the top ``nlevel - 1`` levels), at every wavenumber, in every phase."""
    gcm, cloud = maps
    case = _case(og, calc, gcm)
    t_map = np.repeat(gcm["temperature"][:, :, :-1, None], 7, axis=3)
    case.clouds_4d(dict(cloud, pressure=gcm["pressure"][:-1], opd=t_map), plot=False, verbose=False, calculation=calc)
    tabs = case.inputs["clouds"]["profile_4d"]
    assert len(tabs) == len(PHASES) and np.array_equal(case.inputs["clouds"]["wavenumber"], cloud["wno"])
    for i in range(len(PHASES)):
        want = case.inputs["atmosphere"]["profile_4d"][i]["temperature"][:-1]
        assert tabs[i]["opd"].shape == (want.shape[0], 7, NG, NT)
        for w in range(7):
            assert np.array_equal(tabs[i]["opd"][:, w], want), (calc, i, w)
    assert not np.array_equal(tabs[0]["opd"], tabs[2]["opd"])


@pytest.mark.parametrize("calc", ["reflected", "thermal"])
def test_phase_curve_through_clouds_4d_equals_host_built_curves(og, opa, maps, curves, calc):
    """geometry -> atmosphere_4d(gcm) -> clouds_4d(cloud_gcm) -> phase_curve(opa) equals (i) the curve with
    ``clouds_by_phase=`` the host dictionaries and (ii) every phase alone through phase_angle + atmosphere_3d + clouds_3d +
    spectrum(dimension='3d'); and nothing was copied back on the way."""
    from picaso_amd import justdoit as jdi
    case, curve, untouched, ref_curve, host = curves(calc)
    key = "albedo" if calc == "reflected" else "thermal"
    assert list(curve.keys()) == PHASES and case.inputs["phase_angle"] == PHASES
    assert all(untouched)
    for k, ph in enumerate(PHASES):
        assert np.all(np.isfinite(curve[ph][key]))
        assert np.array_equal(curve[ph][key], ref_curve[ph][key]), (calc, ph)
        one = jdi.inputs()
        one.gravity(gravity=float(og["in/gravity"]))
        one.approx(raman="none")
        one.phase_angle(ph if calc == "reflected" else 0.0, num_gangle=NG, num_tangle=NT)
        one.atmosphere_3d(case.inputs["atmosphere"]["profile_4d"][k])
        one.clouds_3d({a: b.copy() for a, b in host[k].items()})
        want = one.spectrum(opa, calculation=calc, dimension="3d")
        assert np.array_equal(curve[ph][key], want[key]), (calc, ph)
    assert not np.array_equal(curve[PHASES[0]][key], curve[PHASES[2]][key])


@pytest.mark.parametrize("calc", ["reflected", "thermal"])
def test_other_paths_take_the_dictionary_face(og, opa, maps, curves, calc):
    """full_output=True and the facet-fastest layout read ``opd`` / ``w0`` / ``g0`` from the object as from the host
    dictionary: same numbers, and now the host arrays exist."""
    from picaso_amd import justdoit as jdi
    gcm, cloud = maps
    key = "albedo" if calc == "reflected" else "thermal"
    _, curve, _, _, host = curves(calc)
    for kw in (dict(full_output=True), dict(options=jdi.Options(facet_fastest=True))):
        case = _case(og, calc, gcm)
        case.clouds_4d(cloud, plot=False, verbose=False, calculation=calc)
        tabs = case.inputs["clouds"]["profile_4d"]
        assert not any(t.materialized for t in tabs)
        got = case.phase_curve(opa, **kw)
        assert all(t.materialized for t in tabs)
        ref = _case(og, calc, gcm).phase_curve(opa, clouds_by_phase=host, **kw)
        for ph in PHASES:
            assert np.array_equal(got[ph][key], ref[ph][key]), (calc, ph, sorted(kw))
            if "full_output" in kw:
                assert np.array_equal(got[ph][key], curve[ph][key])


def test_correlated_k_tables_read_the_resident_rows(og, maps):
    """A curve on correlated-k tables regrids the cloud rows in wavenumber on the device: from the resident rows as from
    the uploaded host rows, same numbers, nothing copied back."""
    from test_ck_optics import _ck_class
    gcm, cloud = maps
    opk = _ck_class(np.load(os.path.join(GOLDEN, "ck.npz")))
    case = _case(og, "thermal", gcm)
    case.clouds_4d(cloud, plot=False, verbose=False, calculation="thermal")
    got = case.phase_curve(opk)
    assert not any(t.materialized for t in case.inputs["clouds"]["profile_4d"])
    ref_case = _case(og, "thermal", gcm)
    ref = ref_case.phase_curve(opk, clouds_by_phase=_host_by_phase(ref_case, cloud))
    for ph in PHASES:
        assert np.all(np.isfinite(got[ph]["thermal"])) and np.array_equal(got[ph]["thermal"], ref[ph]["thermal"])
    assert not np.array_equal(got[PHASES[0]]["thermal"], got[PHASES[2]]["thermal"])


def test_phase_curve_on_two_devices(og, opa, maps, curves):
    from picaso_amd import _lib
    if _lib.device_count() < 2:
        pytest.skip("needs two visible devices")
    gcm, cloud = maps
    case, curve, _, _, host = curves("thermal")
    got = case.phase_curve(opa, devices=2)
    ref = _case(og, "thermal", gcm).phase_curve(opa, clouds_by_phase=host, devices=2)
    for ph in PHASES:
        assert np.array_equal(got[ph]["thermal"], ref[ph]["thermal"]) and np.array_equal(got[ph]["thermal"], curve[ph]["thermal"])


def test_tables_of_another_device_are_taken_as_the_dictionary(og, opa, maps, curves, monkeypatch):
    """What a phase dealt to another device than the map's does (``devices=N``): the resident face declines, the tables are
    copied back once and go the way of a host dictionary -- same curve."""
    from picaso_amd import gcm as pg
    gcm, cloud = maps
    _, curve, _, _, _ = curves("reflected")
    case = _case(og, "reflected", gcm)
    case.clouds_4d(cloud, plot=False, verbose=False, calculation="reflected")
    monkeypatch.setattr(pg.FacetCloudTables, "resident_tables", lambda self, nlayer, nfac, ctx: None)
    got = case.phase_curve(opa)
    assert all(t.materialized for t in case.inputs["clouds"]["profile_4d"])
    for ph in PHASES:
        assert np.array_equal(got[ph]["albedo"], curve[ph]["albedo"])


def test_chunked_opacity_launches_read_the_resident_rows(og, opa, maps, curves, monkeypatch):
    """A tall atmosphere that takes two gas launches (the table budget holds fewer than all facets): every chunk's rows are
    copied device to device, and the curve is the one-launch curve."""
    from picaso_amd import justdoit as jdi
    from picaso_amd import optics as px
    gcm, cloud = maps
    _, curve, _, _, _ = curves("thermal")
    case = _case(og, "thermal", gcm)
    case.clouds_4d(cloud, plot=False, verbose=False, calculation="thermal")
    launches = []
    real = px._tall_gas_launches

    def two_chunks(opa_, factors, nlayer, nfac):
        whole = px._gas_tables(opa_, factors)
        per_facet = px.gas_table_bytes(len(whole["mol_tabs"]), len(whole["cont_tabs"]), len(whole["ray_tabs"]), nlayer,
                                       whole["cont_wts"])
        monkeypatch.setattr(px, "GAS_TABLE_BUDGET", 4 * per_facet)
        got = list(real(opa_, factors, nlayer, nfac))
        launches.append(len(got))
        return got
    monkeypatch.setattr(px, "_tall_gas_launches", two_chunks)
    got = case.phase_curve(opa, options=jdi.Options(no_driver=True))
    assert launches and min(launches) == 2
    assert not any(t.materialized for t in case.inputs["clouds"]["profile_4d"])
    for ph in PHASES:
        assert np.array_equal(got[ph]["thermal"], curve[ph]["thermal"])


def test_second_clouds_4d_uploads_nothing(og, maps, curves):
    """Residency: the same arrays again (copies of them, even) come from the same resident map."""
    from picaso_amd import gcm as pg
    gcm, cloud = maps
    case, _, _, _, _ = curves("thermal")
    first = case.inputs["clouds"]["profile_4d"][0].map
    before = pg.UPLOADS
    case.clouds_4d({k: np.array(v, copy=True) for k, v in cloud.items()}, plot=False, verbose=False, calculation="thermal")
    assert pg.UPLOADS == before and all(t.map is first for t in case.inputs["clouds"]["profile_4d"])
    edited = dict(cloud, w0=cloud["w0"] * 0.5)
    case.clouds_4d(edited, plot=False, verbose=False, calculation="thermal")
    assert pg.UPLOADS == before + 1 and case.inputs["clouds"]["profile_4d"][0].map is not first


def test_clouds_by_phase_wins_and_clouds_reset_clears(og, opa, maps, curves):
    gcm, cloud = maps
    _, curve, _, ref_curve, host = curves("thermal")
    case = _case(og, "thermal", gcm)
    case.clouds_4d(dict(cloud, opd=cloud["opd"] * 3.0), plot=False, verbose=False, calculation="thermal")
    thick = case.phase_curve(opa)
    assert not np.array_equal(thick[PHASES[1]]["thermal"], curve[PHASES[1]]["thermal"])
    explicit = case.phase_curve(opa, clouds_by_phase=host)
    for ph in PHASES:
        assert np.array_equal(explicit[ph]["thermal"], ref_curve[ph]["thermal"])
    case.clouds_reset()
    assert "profile_4d" not in case.inputs["clouds"]
    clear = case.phase_curve(opa)
    want = _case(og, "thermal", gcm).phase_curve(opa)
    for ph in PHASES:
        assert np.array_equal(clear[ph]["thermal"], want[ph]["thermal"])
        assert not np.array_equal(clear[ph]["thermal"], curve[ph]["thermal"])
