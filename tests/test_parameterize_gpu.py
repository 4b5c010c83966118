"""``picaso_param_cloud_tables_dev`` (csrc/paramcloud.hip) and its Python face on the GPU: the rows of one launch against
the reference's tables (tests/golden/parameterizations.npz), batch independence, the C entry's refusals, the two faces of
``ParamCloudTable``, and spectra fed from tables made in HBM against the same spectra fed the same values as dictionaries.

With every ``alpha = 0`` the rows are the reference's bits.  With ``alpha != 0`` they are held to a bound that follows
from how the element is formed, in units of u = 2^-53:

    ratio = wavelength / reference_wave      one IEEE division: u, which the power turns into |alpha| u
    power = pow(ratio, -alpha)               the device library's pow, 1 ulp <= 2 u
    opd_k = opd_l * power                    one product: u
    opd   = sum of K terms                   K - 1 sums of non-negative terms: (K - 1) u

so opd is within (|alpha| + 2 + K) u of the exact value, and the averaged w0 and g0 within twice that of
``sum(opd_k |g0_k|) / opd`` (their numerator and their denominator each carry the error once).  The yardstick is the same
expression in ``np.longdouble``, written here.  The largest distances measured on an MI355X (this file, in u): reference
fp64 vs yardstick 2.91 (opd) and 2.78 of their scale (w0 / g0); device vs yardstick 3.09 and 2.96 -- DESIGN.md 5n."""
import ctypes
import os

import numpy as np
import pytest

from test_devices_gpu import _same
from test_optics import DB
from test_parameterize_host import AVG_CASES, CASES, Z, avg_decks, make_param, write_grid

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
POW_ULP = 1.0                     # the device library's double-precision pow: 1 ulp (HIP's published accuracy table)
SECOND_ORDER = 1.0 + 2.0 ** -40   # the products of the u's above


def launch(layers, params, wavelength, average, S=None, K=None, nlayer=None, nin=None, null=None, out=None):
    """One call of the C entry on host arrays: ``(return code, (S, 3, nlayer, nin) rows or the untouched ``out``)``."""
    from picaso_amd import _lib, device
    from picaso_amd.device import DeviceArray
    ctx = _lib.context()
    layers, params, wavelength = (np.ascontiguousarray(x, dtype=np.float64) for x in (layers, params, wavelength))
    s_, k_, _, nl_ = layers.shape
    S, K, nlayer, nin = (d if v is None else v for v, d in ((S, s_), (K, k_), (nlayer, nl_), (nin, wavelength.size)))
    d_in = [DeviceArray.from_host(x, ctx) for x in (layers, params, wavelength)]
    d_out = out if out is not None else DeviceArray.zeros((s_, 3, nl_, wavelength.size), ctx)
    addrs = [d.addr for d in d_in] + [d_out.addr]
    if null is not None:
        addrs[null] = None
    rc = _lib.load().picaso_param_cloud_tables_dev(ctx, S, K, nlayer, nin, average, *addrs)
    device.sync(ctx)
    return rc, d_out.to_host()


def yardstick(decks, wavelength, average):
    """The kernel's expression in ``np.longdouble`` from the same inputs: ``(opd, w0, g0, sum(opd_k |w0_k|) / opd,
    sum(opd_k |g0_k|) / opd)``."""
    L = np.longdouble
    wl = np.asarray(wavelength, dtype=L)
    terms = [np.asarray(d[0], dtype=L)[:, None] * ((wl / L(d[4])) ** L(-d[3]))[None, :] for d in decks]
    if not average:
        one = np.ones_like(terms[0])
        return terms[0], np.asarray(decks[0][1], dtype=L)[:, None] * one, np.asarray(decks[0][2], dtype=L)[:, None] * one, None, None
    opd = sum(terms)
    num = [sum(t * np.asarray(d[j], dtype=L)[:, None] for t, d in zip(terms, decks)) for j in (1, 2)]
    mag = [sum(t * np.abs(np.asarray(d[j], dtype=L))[:, None] for t, d in zip(terms, decks)) for j in (1, 2)]
    opd = np.where(opd == 0, L(1e-33), opd)
    return opd, num[0] / opd, num[1] / opd, mag[0] / opd, mag[1] / opd


def held(got, ref, decks, wavelength, average, tag):
    """``got`` (device rows) against the yardstick at the derived bound; prints the reference's own and the device's
    largest distance in units of the bound's scale times u.  Returns those two pairs."""
    K = len(decks)
    exact = yardstick(decks, wavelength, average)
    budget = (max(abs(d[3]) for d in decks) + 2.0 * POW_ULP + K) * U * SECOND_ORDER
    figures = []
    for j, name in enumerate(("opd", "w0", "g0")):
        x = exact[j]
        if j == 0:
            scale, allowed = np.abs(x), budget
        elif average:
            scale, allowed = exact[2 + j], 2.0 * budget
        else:
            assert np.array_equal(got[j], np.asarray(x, dtype=np.float64)), (tag, name)       # stored as they are
            continue
        safe = np.where(scale == 0, 1, scale)
        d_dev = np.max(np.where(scale == 0, np.abs(got[j] - x), np.abs(got[j] - x) / safe))
        d_ref = np.max(np.where(scale == 0, np.abs(ref[j] - x), np.abs(ref[j] - x) / safe))
        print("%s %s: reference fp64 vs yardstick %.2f u, device vs yardstick %.2f u, allowed %.2f u"
              % (tag, name, float(d_ref) / U, float(d_dev) / U, allowed / U))
        assert np.all(np.abs(got[j] - x) <= allowed * scale), (tag, name, float(d_dev) / U, allowed / U)
        figures.append((name, float(d_ref) / U, float(d_dev) / U))
    return figures


GREY = [c for c in CASES if c["fn"] == "cloud_brewster_grey"]


def test_single_decks_against_the_reference(tmp_path, monkeypatch):
    """average = 0 through ``cloud_tables_batch``: every ``cloud_brewster_grey`` case of the fixture, all cases of a shape
    in one launch; ``alpha = 0`` bit for bit, the others at the bound.  The box clouds on the 196-point grid too."""
    for nl, nin in sorted({(c["nlayer"], c["nin"]) for c in GREY}):
        grid = write_grid(tmp_path, monkeypatch, nin)
        p = make_param(nl)
        cases = [c for c in GREY if (c["nlayer"], c["nin"]) == (nl, nin)]
        tabs = p.cloud_tables_batch([[dict(c["kwargs"], kind="brewster_grey")] for c in cases])
        assert len(tabs) == len(cases) and all(t.d_stack.shape == (3 * nl, nin) for t in tabs)
        for c, t in zip(cases, tabs):
            got = t.d_stack.to_host().reshape(3, nl, nin)
            ref = [Z["out/%s/%s" % (c["name"], k)].reshape(nl, nin) for k in ("opd", "w0", "g0")]
            kw = c["kwargs"]
            if kw["alpha"] == 0:
                assert all(np.array_equal(g, r) for g, r in zip(got, ref)), c["name"]
                continue
            opd_l = p._grey_layers(kw["decay_type"], kw.get("slab_kwargs"), kw.get("deck_kwargs"))
            deck = (opd_l, np.full(nl, kw["ssa"]), np.zeros(nl), kw["alpha"], kw["reference_wave"])
            held(got, ref, [deck], 1e4 / grid, 0, c["name"])
    write_grid(tmp_path, monkeypatch, 196)
    p = make_param(5)
    for c in (c for c in CASES if c["fn"] == "cloud_hard_grey"):
        t = p.cloud_hard_grey(out="device", **c["kwargs"])
        got = t.d_stack.to_host().reshape(3, 5, 196)
        for j, k in enumerate(("opd", "w0", "g0")):
            assert np.array_equal(got[j], Z["out/%s/%s" % (c["name"], k)].reshape(5, 196)), (c["name"], k)


@pytest.mark.parametrize("name", AVG_CASES)
def test_averaged_decks_against_the_reference(name):
    """average = 1 through the C entry with the fixture's deck records (w0 and g0 per layer, g0 of mixed sign, nothing in
    the top layer: the 1e-33 branch): all ``alpha = 0`` bit for bit, the others at the bound."""
    decks = avg_decks(name)
    nl, nin = decks[0][5].shape
    wavelength = 1e4 / Z["grid/%d" % nin]
    layers = np.array([[d[0], d[1], d[2]] for d in decks])[None]
    params = np.array([[d[3], d[4]] for d in decks])[None]
    rc, rows = launch(layers, params, wavelength, 1)
    assert rc == 0
    got = rows[0]
    ref = [Z["avg/%s/%s" % (name, k)] for k in ("opd", "w0", "g0")]
    assert np.all(got[0][0] == 1e-33) and not np.any(got[1][0]) and not np.any(got[2][0])
    if all(d[3] == 0 for d in decks):
        assert all(np.array_equal(g, r) for g, r in zip(got, ref)), name
    else:
        figures = held(got, ref, decks, wavelength, 1, name)
        assert len(figures) == 3
    for k, d in enumerate(decks):                      # each deck alone, stored as it is: the deck's own table
        rc, rows = launch(layers[:, k:k + 1], params[:, k:k + 1], wavelength, 0)
        assert rc == 0
        if d[3] == 0:
            assert np.array_equal(rows[0][0], d[5])
        else:
            held(rows[0], [d[5], None, None], [d], wavelength, 0, "%s deck %d" % (name, k))


def test_batch_members_do_not_depend_on_the_batch():
    """S = 5 in one launch equals the five S = 1 launches bit for bit, for K = 1 .. 4, on 37 layers x 67 wavenumbers; the
    same for five members of S = 400 on 90 layers x 7 wavenumbers, where a workgroup takes 32 layers and not one (the
    host deals out more than one layer from S x nlayer = 2048 on) -- and a sample filled up with empty decks equals the
    sample launched with its own K."""
    rng = np.random.default_rng(11)
    for nl, nin, S in ((37, 67, 5), (90, 7, 400)):
        wavelength = 1e4 / np.sort(rng.uniform(50.0, 30000.0, nin))
        for K in (1, 2, 3, 4):
            layers = rng.random((S, K, 3, nl)) * 10.0 ** rng.integers(-6, 2, (S, K, 3, 1))
            layers[:, :, 2] = rng.uniform(-1, 1, (S, K, nl))
            layers[:, :, 0, :3] = 0.0
            params = np.stack([rng.choice([0.0, 1.5, -0.7, 3.2], (S, K)), rng.uniform(0.5, 3.0, (S, K))], axis=-1)
            for average in ((0, 1) if K == 1 else (1,)):
                rc, together = launch(layers, params, wavelength, average)
                assert rc == 0 and np.all(np.isfinite(together))
                for s in list(range(S))[:5]:
                    rc, alone = launch(layers[s:s + 1], params[s:s + 1], wavelength, average)
                    assert rc == 0 and np.array_equal(alone[0], together[s]), (nl, nin, K, average, s)
            if K < 4:                                  # filled up to 4 decks with empty ones (alpha 0, reference_wave 1)
                pad_l, pad_p = np.zeros((S, 4, 3, nl)), np.zeros((S, 4, 2))
                pad_p[:, :, 1] = 1.0
                pad_l[:, :K], pad_p[:, :K] = layers, params
                rc, padded = launch(pad_l, pad_p, wavelength, 1)
                rc2, own = launch(layers, params, wavelength, 1)
                assert rc == 0 and rc2 == 0 and np.array_equal(padded, own), (nl, nin, K)


def test_wide_grid_takes_more_than_one_tile():
    """nin = 661 (the climate tables' grid) is two tiles of wavelengths, the second narrower than a workgroup: the rows
    against numpy's own evaluation at ``alpha = 0`` (exact) and the yardstick otherwise."""
    rng = np.random.default_rng(12)
    nl, nin = 9, 661
    wavelength = 1e4 / np.linspace(30.0, 33000.0, nin)
    layers = rng.random((2, 2, 3, nl))
    params = np.array([[[0.0, 1.0], [0.0, 2.0]], [[1.5, 1.0], [-0.7, 2.3]]])
    rc, rows = launch(layers, params, wavelength, 1)
    assert rc == 0
    opd = layers[0, 0, 0] + layers[0, 1, 0]
    w0 = (layers[0, 0, 0] * layers[0, 0, 1] + layers[0, 1, 0] * layers[0, 1, 1]) / opd
    assert np.array_equal(rows[0][0], np.repeat(opd[:, None], nin, axis=1))
    assert np.array_equal(rows[0][1], np.repeat(w0[:, None], nin, axis=1))
    decks = [(layers[1, k, 0], layers[1, k, 1], layers[1, k, 2], params[1, k, 0], params[1, k, 1]) for k in range(2)]
    numpy_rows = yardstick(decks, wavelength, 1)[:3]
    held(rows[1], [np.asarray(x, dtype=np.float64) for x in numpy_rows], decks, wavelength, 1, "661 wavenumbers")


def test_the_c_entry_refuses_bad_arguments_and_launches_nothing():
    from picaso_amd import _lib
    from picaso_amd.device import DeviceArray
    ctx = _lib.context()
    nl, nin = 4, 5
    layers, params, wavelength = np.ones((1, 1, 3, nl)), np.array([[[1.5, 1.0]]]), np.linspace(1.0, 5.0, nin)
    mark = np.full((1, 3, nl, nin), -7.0)
    out = DeviceArray.from_host(mark, ctx)
    bad = [dict(nin=1), dict(nin=0), dict(K=0), dict(K=5), dict(nlayer=0), dict(S=0), dict(S=-3), dict(null=0), dict(null=1),
           dict(null=2), dict(null=3), dict(average=2)]
    for kw in bad:
        average = kw.pop("average", 0)
        rc, rows = launch(layers, params, wavelength, average, out=out, **kw)
        assert rc != 0 and np.array_equal(rows, mark), kw
        assert b"picaso_param_cloud_tables_dev" in _lib.load().picaso_last_error(ctx), kw
    rc, rows = launch(np.ones((1, 2, 3, nl)), np.ones((1, 2, 2)), wavelength, 0, out=out)      # two decks, stored as they are
    assert rc != 0 and np.array_equal(rows, mark)
    assert _lib.load().picaso_param_cloud_tables_dev(None, 1, 1, nl, nin, 0, None, None, None, None) != 0
    rc, rows = launch(layers, params, wavelength, 0, out=out)
    assert rc == 0 and not np.any(rows == -7.0)
    p = make_param(5)
    with pytest.raises(ValueError, match="1 to 4 decks"):
        p.cloud_tables_batch([[]])
    with pytest.raises(ValueError, match="average=0"):
        p.cloud_tables_batch([[dict(kind="hard_grey", g0=0, w0=1, opd=1, p=0, dp=1)] * 2], average=0)
    assert p.cloud_tables_batch([]) == []


# ---- end to end, on the small opacity object the other GPU tests use
@pytest.fixture(scope="module")
def og():
    from helpers import GOLDEN
    return np.load(os.path.join(GOLDEN, "optics.npz"))


@pytest.fixture(scope="module")
def opa():
    from picaso_amd import justdoit as jdi
    return jdi.opannection(filename_db=DB, query_method="linear")


def _cloud_grid(tmp_path, monkeypatch, og):
    """A 67-point cloud grid inside the opacity grid as ``wave_EGP.dat``."""
    d = tmp_path / "opacities"
    d.mkdir(exist_ok=True)
    wno = og["in/wno"]
    grid = np.round(np.geomspace(wno.min() * 1.02, wno.max() * 0.97, 67), 2)
    with open(d / "wave_EGP.dat", "w") as fh:
        fh.write("   i   wavenumber\n")
        for i, w in enumerate(grid[::-1]):
            fh.write("%4d %.2f\n" % (i + 1, w))
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    return grid


def _case(og, clouds=None, k=0):
    from picaso_amd import justdoit as jdi
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=float(og["in/gravity"]), radius=7.1e9, mass=1.9e30)
    prof = {"pressure": og["in/plevel_bar"], "temperature": og["in/tlevel"] * (1.0 + 0.01 * k)}
    for m in ("H2", "He", "H2O", "CH4"):
        prof[m] = og["in/mix/" + m]
    case.atmosphere(df=prof)
    nwno = len(og["in/wno"])
    case.star(relative_flux=1.0 + 0.2 * np.cos(np.arange(nwno) / 5.0), radius=6.9e10, semi_major=7.5e12)
    case.approx(raman="none")
    if clouds is not None:
        case.clouds(df=clouds)
    return case


def _samples(og, n):
    """``n`` samples of a two-deck cloud on the profile's pressure grid: a slab above a deck, parameters moving."""
    lo, hi = np.log10(og["in/plevel_bar"][[0, -1]])
    out = []
    for k in range(n):
        out.append([dict(kind="brewster_grey", decay_type="slab", alpha=1.5 - 0.4 * k, ssa=0.9, reference_wave=1.0,
                         slab_kwargs=dict(ptop=lo + 0.25 * (hi - lo), dp=0.3 * (hi - lo), reference_tau=0.5 + 0.2 * k)),
                    dict(kind="brewster_grey", decay_type="deck", alpha=0.0, ssa=0.5 + 0.05 * k, reference_wave=1.0,
                         deck_kwargs=dict(ptop=lo + 0.8 * (hi - lo), dp=0.5))])
    return out


def test_faces_and_spectrum(tmp_path, monkeypatch, og, opa):
    """The dictionary face is the device rows; ``clouds(df=table)`` gives the spectrum of ``clouds(df=dict(table))`` bit for
    bit, without a cloud upload where the dictionary needs one; a table relabelled to (or made on) another device falls back
    to its dictionary face and still agrees."""
    from picaso_amd import _lib, optics
    from picaso_amd import parameterizations as pz
    grid = _cloud_grid(tmp_path, monkeypatch, og)
    p = pz.Parameterize()
    p.add_class(_case(og))
    nl = p.nlayer
    table = p.cloud_tables_batch(_samples(og, 1))[0]
    assert isinstance(table, pz.ParamCloudTable) and not table.materialized
    assert table.d_xp.shape == (67,) and np.array_equal(table.d_xp.to_host(), grid) and table.d_stack.shape == (3 * nl, 67)
    assert table.stamp[:2] == p._resident_grids(None)["digest"] and all(isinstance(v, float) for d in table.stamp[3] for v in d)
    rows = table.d_stack.to_host().reshape(3, nl, 67)
    assert np.any(rows[0] > 0) and np.all(np.isfinite(rows))

    before = optics.CLOUD_UPLOADS
    got = _case(og, table).spectrum(opa, calculation="reflected+thermal")
    assert optics.CLOUD_UPLOADS == before and not table.materialized
    plain = dict(table)
    assert table.materialized and type(plain) is dict
    for j, k in enumerate(("opd", "w0", "g0")):
        assert np.array_equal(plain[k].reshape(nl, 67), rows[j]), k
    assert np.array_equal(plain["wavenumber"], np.tile(grid, nl))
    want = _case(og, plain).spectrum(opa, calculation="reflected+thermal")
    assert optics.CLOUD_UPLOADS == before + 1
    _same(got, want)
    assert np.all(np.isfinite(got["albedo"])) and np.all(np.isfinite(got["thermal"]))
    free = _case(og).spectrum(opa, calculation="reflected+thermal")
    assert not np.array_equal(free["albedo"], got["albedo"])            # the cloud is seen

    # one deck through out='device' is the DataFrame's table where alpha = 0
    deck = dict(decay_type="deck", alpha=0, ssa=0.7, deck_kwargs=dict(ptop=-1.0, dp=0.5))
    df = p.cloud_brewster_grey(**deck)
    dev = p.cloud_brewster_grey(out="device", **deck)
    for k in ("opd", "w0", "g0", "wavenumber", "pressure"):
        assert np.array_equal(dev[k], df[k].values), k

    # another device: really, where there is one; else the table relabelled to a device this machine does not have
    other = pz.Parameterize()
    other.add_class(_case(og))
    sample = _samples(og, 2)[1:]                       # (another cloud: the opacity object remembers the last upload's content)
    if _lib.device_count() > 1:
        away = other.cloud_tables_batch(sample, ctx=_lib.context(1))[0]
    else:
        away = other.cloud_tables_batch(sample)[0]
        away.resident = dict(away.resident, ctx=ctypes.c_void_p(1), device=_lib.device_of(opa.ctx) + 1)
    assert away.resident_tables(nl, opa.ctx) is None and table.resident_tables(nl, opa.ctx) is not None
    assert table.resident_tables(nl + 1, opa.ctx) is None
    before = optics.CLOUD_UPLOADS
    fell = _case(og, away).spectrum(opa, calculation="reflected+thermal")
    assert optics.CLOUD_UPLOADS == before + 1 and away.materialized
    _same(fell, _case(og, dict(away)).spectrum(opa, calculation="reflected+thermal"))
    assert not np.array_equal(fell["albedo"], want["albedo"])


def test_spectrum_batch_from_one_launch(tmp_path, monkeypatch, og, opa):
    """Five cases whose tables are views of one launch through ``spectrum_batch`` against the same cases fed the tables as
    dictionaries: bit for bit, no cloud upload against five; and once with ``full_output=True``, where the host face is
    read."""
    from picaso_amd import justdoit as jdi
    from picaso_amd import optics
    from picaso_amd import parameterizations as pz
    _cloud_grid(tmp_path, monkeypatch, og)
    p = pz.Parameterize()
    p.add_class(_case(og))
    launches = pz.LAUNCHES
    tabs = p.cloud_tables_batch(_samples(og, 5))
    assert pz.LAUNCHES == launches + 1 and len(tabs) == 5
    assert len({t.d_stack.addr for t in tabs}) == 5 and all(t.d_stack._owner is tabs[0].d_stack._owner for t in tabs)
    before = optics.CLOUD_UPLOADS
    got = jdi.spectrum_batch([_case(og, t, k) for k, t in enumerate(tabs)], opa, calculation="reflected+thermal")
    assert optics.CLOUD_UPLOADS == before and not any(t.materialized for t in tabs)
    want = jdi.spectrum_batch([_case(og, dict(t), k) for k, t in enumerate(tabs)], opa, calculation="reflected+thermal")
    assert optics.CLOUD_UPLOADS == before + 5
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        _same(g, w)
    assert not np.array_equal(got[0]["albedo"], got[4]["albedo"])
    full = jdi.spectrum_batch([_case(og, t, k) for k, t in enumerate(tabs[:2])], opa, calculation="reflected+thermal",
                              full_output=True)
    full_want = jdi.spectrum_batch([_case(og, dict(t), k) for k, t in enumerate(tabs[:2])], opa,
                                   calculation="reflected+thermal", full_output=True)
    for g, w in zip(full, full_want):
        _same(g, w)
        for k in ("opd", "w0", "g0"):
            assert np.array_equal(g["full_output"]["layer"]["cloud"][k], w["full_output"]["layer"]["cloud"][k]), k
