"""``picaso_amd.parameterizations`` against the reference's own functions (tests/golden/parameterizations.npz, written by
tests/golden/make_parameterizations.py): every built form of ``Parameterize``, ``atlev``, ``picaso_format`` and
``cloud_averaging``; the refusals; and the dictionary, copy and pickle behaviour of ``ParamCloudTable`` on a stub.

Forms that are numpy arithmetic only must give the fixture's bits.  Forms that go through scipy (``pt_knots``,
``pt_zj24``, ``vmr_knots`` and the ``chem_free`` that calls it, ``pt_guillot``) must give them under the scipy version
that wrote the fixture; under another version they are held to 2^-40 relative -- a margin against another spline or
``expn`` build, not an accuracy claim -- and the test says so in its output."""
import copy
import json
import os
import pickle

import numpy as np
import pytest

from helpers import GOLDEN
from picaso_amd import justdoit as jdi
from picaso_amd import parameterizations as pz

Z = np.load(os.path.join(GOLDEN, "parameterizations.npz"))
CASES = json.loads(str(Z["cases"]))
SCIPY_FORMS = ("pt_knots", "pt_zj24", "vmr_knots", "pt_guillot")
FORMAT_CASES = sorted({k.split("/")[1] for k in Z.files if k.startswith("format/")})
AVG_CASES = sorted({k.split("/")[1] for k in Z.files if k.startswith("avg/")})


def write_grid(tmp_path, monkeypatch, nin):
    """The fixture's ``nin``-point cloud grid as ``$picaso_refdata/opacities/wave_EGP.dat`` (decreasing, as the real file)."""
    d = tmp_path / "opacities"
    d.mkdir(exist_ok=True)
    grid = Z["grid/%d" % nin]
    with open(d / "wave_EGP.dat", "w") as fh:
        fh.write("   i   wavenumber\n")
        for i, w in enumerate(grid[::-1]):
            fh.write("%4d %.2f\n" % (i + 1, w))
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    assert np.array_equal(jdi.get_cld_input_grid(), grid)
    return grid


def make_param(nlayer, temperature=False, gravity=None):
    case = jdi.inputs()
    case.add_pt(T=Z["tlevel/12"] if temperature else None, P=Z["plevel/%d" % nlayer])
    if gravity is not None:
        case.gravity(gravity=gravity)
    p = pz.Parameterize()
    p.add_class(case)
    return p


def _uses_scipy(case):
    if case["fn"] in SCIPY_FORMS:
        return True
    return case["fn"] == "chem_free" and any(isinstance(v, dict) and v.get("profile") == "knots"
                                             for v in case["kwargs"].values())


def _same(got, want, scipy_form, tag):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, tag
    if np.array_equal(got, want):
        return
    import scipy
    recorded = str(Z["meta/scipy"])
    assert scipy_form and scipy.__version__ != recorded, (tag, "differs from the fixture", np.max(np.abs(got - want)))
    rel = np.max(np.abs(got - want) / np.abs(want))
    print("%s: scipy %s here, %s wrote the fixture: not bit for bit, held to 2^-40 relative (found %.3g)"
          % (tag, scipy.__version__, recorded, rel))
    assert rel <= 2.0 ** -40, (tag, rel)


def test_add_class_sets_the_reference_attributes():
    p = make_param(12, temperature=True, gravity=2200.0)
    plev = Z["plevel/12"]
    assert np.array_equal(p.pressure_level, plev) and np.array_equal(p.temperature_level, Z["tlevel/12"])
    assert np.array_equal(p.pressure_layer, np.sqrt(plev[0:-1] * plev[1:]))
    assert (p.nlevel, p.nlayer, p.gravity_cgs) == (13, 12, 2200.0) and isinstance(p.picaso, jdi.inputs)
    bare = make_param(5)
    assert len(bare.temperature_level) == 0 and np.isnan(bare.gravity_cgs)
    with pytest.raises(AssertionError, match="t grid"):
        bare.chem_free(H2O=dict(value=1e-4))
    with pytest.raises(AssertionError, match="not supplied"):
        bare.pt_guillot(1000.0, 100.0, -1.0, -2.0, 0.5)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_against_the_reference(case, tmp_path, monkeypatch):
    write_grid(tmp_path, monkeypatch, case["nin"])
    p = make_param(case["nlayer"], **case["how"])
    fn = getattr(p, case["fn"])
    if case["raises"]:
        with pytest.raises(Exception, match="not large enough"):
            fn(**case["kwargs"])
        return
    out = fn(**case["kwargs"])
    prefix = "out/%s/" % case["name"]
    want = {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix)}
    assert want
    if list(want) == ["value"]:
        _same(out, want["value"], _uses_scipy(case), case["name"])
        return
    assert sorted(out.columns) == sorted(want), case["name"]
    for col, ref in want.items():
        _same(out[col].values, ref, _uses_scipy(case), "%s/%s" % (case["name"], col))


def test_shapes_are_the_per_layer_loops():
    """``deck_decay`` and ``slab_decay`` vectorised over layers against the reference's own form written out here -- a loop
    over ``atlev`` with numpy scalars -- on random ``(ptop, dp)``, slab exceptions included."""
    rng = np.random.default_rng(3)
    p = make_param(12)
    pl = p.pressure_layer
    for ptop, dp in zip(rng.uniform(-6.5, 2.5, 120), 10 ** rng.uniform(-3, 0.7, 120)):
        ptp = 10 ** ptop
        scale = ((ptp * 10. ** dp) - ptp) / 10. ** dp
        const = 1. / (1 - np.exp(-ptp / scale))
        want = np.zeros(12)
        for i in range(12):
            t, b = pz.atlev(i, pl)
            t1, t2 = (b - ptp) / scale, (t - ptp) / scale
            want[i] = 100.0 if (t1 > 10 or t2 > 10) else const * (np.exp(t1) - np.exp(t2))
        assert np.array_equal(p.deck_decay(ptop, dp), want, equal_nan=True), (ptop, dp)
        pb = ptp * 10. ** dp
        it, ib = np.argmin(abs(np.log(pl) - np.log(ptp))), np.argmin(abs(np.log(pl) - np.log(pb)))
        if it == ib:
            with pytest.raises(Exception, match="not large enough"):
                p.slab_decay(ptop, dp, 1.7)
            continue
        want = np.zeros(12)
        sc = 1.7 / (pb ** 2 - ptp ** 2)
        want[it] = sc * (pz.atlev(it, pl)[1] ** 2 - ptp ** 2)
        want[ib] = sc * (pb ** 2 - pz.atlev(ib, pl)[0] ** 2)
        for i in range(it + 1, ib):
            t, b = pz.atlev(i, pl)
            want[i] = sc * (b ** 2 - t ** 2)
        assert np.array_equal(p.slab_decay(ptop, dp, 1.7), want), (ptop, dp)


@pytest.mark.parametrize("name", FORMAT_CASES)
def test_picaso_format(name):
    pre = "format/%s/" % name
    nl, nin = (int(x) for x in name.rsplit("_", 1)[1].split("x"))
    plev = Z["plevel/%d" % nl]
    kw = {}
    for k in Z.files:
        if k.startswith(pre + "kw_"):
            v = Z[k]
            kw[k[len(pre) + 3:]] = v if v.ndim else float(v)
    out = pz.picaso_format(Z[pre + "in_opd"], Z[pre + "in_w0"], Z[pre + "in_g0"], Z["grid/%d" % nin],
                           np.sqrt(plev[0:-1] * plev[1:]), **kw)
    assert list(out.columns) == ["pressure", "wavenumber", "opd", "w0", "g0"]
    for c in out.columns:
        assert np.array_equal(np.asarray(out[c].values, dtype=np.float64), Z[pre + c]), (name, c)
    with pytest.raises(Exception, match="Must specify"):
        pz.picaso_format(Z[pre + "in_opd"], Z[pre + "in_w0"], Z[pre + "in_g0"], Z["grid/%d" % nin], plev[1:])


def avg_decks(name):
    """The deck records of one cloud_averaging case: ``[(opd_l, w0_l, g0_l, alpha, reference_wave, the deck's table)]``."""
    decks, k = [], 0
    while "avg/%s/d%d/opd_l" % (name, k) in Z.files:
        pre = "avg/%s/d%d/" % (name, k)
        decks.append(tuple(Z[pre + x] for x in ("opd_l", "w0_l", "g0_l")) + (float(Z[pre + "alpha"]),
                                                                             float(Z[pre + "reference_wave"]), Z[pre + "opd"]))
        k += 1
    return decks


@pytest.mark.parametrize("name", AVG_CASES)
def test_cloud_averaging(name):
    import pandas as pd
    decks = avg_decks(name)
    nl, nin = decks[0][5].shape
    dfs = [pd.DataFrame({"opd": d[5].reshape(-1), "w0": np.repeat(d[1], nin), "g0": np.repeat(d[2], nin)}) for d in decks]
    out = pz.cloud_averaging(dfs)
    assert out is dfs[0]
    for c in ("opd", "w0", "g0"):
        assert np.array_equal(out[c].values.reshape(nl, nin), Z["avg/%s/%s" % (name, c)]), (name, c)
    assert np.all(out["opd"].values[:nin] == 1e-33)
    with pytest.raises(AssertionError, match="different grids"):
        pz.cloud_averaging([dfs[0], dfs[1].iloc[:-1]])


def test_refused_forms_say_what_is_missing():
    with pytest.raises(NotImplementedError, match="virga"):
        pz.Parameterize(load_cld_optical="SiO2", mieff_dir="/somewhere")
    with pytest.raises(NotImplementedError, match="virga"):
        pz.Parameterize(mieff_dir="/somewhere")
    p = make_param(5)
    for fn, word in (("cloud_virga", "virga"), ("cloud_flex_fsed", "calc_optics_user_r_dist"), ("flex_cloud", "calc_optics"),
                     ("cloud_brewster_mie", "Mie"), ("pt_madhu_seager_09_noinversion", "astropy"),
                     ("pt_madhu_seager_09_inversion", "astropy")):
        with pytest.raises(NotImplementedError, match=word):
            getattr(p, fn)()
    with pytest.raises(NotImplementedError, match="chemeq_visscher_2121"):
        p.chem_visscher(0.55, 0.0)
    with pytest.raises(NotImplementedError, match="scipy.interpolate"):
        p.pt_knots([1e-3, 1.0], [500.0, 900.0], interpolation="PchipInterpolator")
    with pytest.raises(Exception, match="Unknown interpolation"):
        p.pt_knots([1e-3, 1.0], [500.0, 900.0], interpolation="no_such_thing")
    with pytest.raises(AssertionError, match="at least 4"):
        p.pt_knots([1e-3, 1.0, 10.0], [500.0, 900.0, 950.0], interpolation="cubic_spline")


# ---- ParamCloudTable without a device: a stub of the rows in HBM
class _StubRows:
    def __init__(self, rows):
        self.rows, self.copies = rows, 0

    def to_host(self):
        self.copies += 1
        return self.rows.copy()


def _stub_table(nlayer=3, nin=7):
    rng = np.random.default_rng(1)
    rows = _StubRows(rng.random((3 * nlayer, nin)))
    grid = Z["grid/%d" % nin]
    player = np.sqrt(Z["plevel/%d" % nlayer][:-1] * Z["plevel/%d" % nlayer][1:])
    res = dict(ctx=None, grid=grid, d_xp=object(), d_wave=object(), device=0, digest=(b"p", b"w"))
    return pz.ParamCloudTable(res, player, rows, nlayer, (b"p", b"w", 0, ((0.0, 1.0),))), rows, grid, player


def test_param_cloud_table_dictionary_face():
    t, rows, grid, player = _stub_table()
    assert isinstance(t, dict) and not t.materialized and rows.copies == 0
    assert len(t) == 5 and "opd" in t and "pressure" in t and "tau" not in t and rows.copies == 0
    r3 = rows.rows.reshape(3, 3, 7)
    assert np.array_equal(t["w0"], r3[1].reshape(-1)) and t.materialized and rows.copies == 1
    assert np.array_equal(t["opd"], r3[0].reshape(-1)) and np.array_equal(t.get("g0"), r3[2].reshape(-1))
    assert np.array_equal(t["wavenumber"], np.tile(grid, 3)) and np.array_equal(t["pressure"], np.repeat(player, 7))
    assert sorted(t.keys()) == sorted(["opd", "w0", "g0", "wavenumber", "pressure"]) and rows.copies == 1
    assert t.get("tau") is None
    plain = dict(t)
    assert type(plain) is dict and sorted(plain) == sorted(t.keys()) and np.array_equal(plain["opd"], t["opd"])
    fresh = _stub_table()[0]
    assert sorted(dict(fresh)) == sorted(plain) and fresh.materialized      # dict() of an untouched table fills it
    for edit in (lambda: t.__setitem__("opd", 0), lambda: t.update(opd=0), lambda: t.pop("opd"), lambda: t.clear(),
                 lambda: t.__delitem__("opd"), lambda: t.setdefault("x", 1), lambda: t.popitem()):
        with pytest.raises(TypeError, match="not editable"):
            edit()
    assert np.array_equal(t["opd"], r3[0].reshape(-1))


def test_param_cloud_table_copy_and_pickle():
    t, rows, _, _ = _stub_table()
    assert copy.deepcopy(t) is t and copy.copy(t) is t and copy.deepcopy({"profile": t})["profile"] is t
    assert rows.copies == 0
    back = pickle.loads(pickle.dumps(t))
    assert type(back) is dict and sorted(back) == sorted(["opd", "w0", "g0", "wavenumber", "pressure"])
    assert all(np.array_equal(back[k], t[k]) for k in back) and rows.copies == 1
    c = t.copy()
    assert type(c) is dict and np.array_equal(c["g0"], t["g0"])


def test_clouds_keeps_the_table_and_get_clouds_hands_it_on():
    """``inputs.clouds(df=table)`` stores the object; ``ATMSETUP.get_clouds`` makes a ``CloudTables`` that carries it and
    forms ``compact`` from the dictionary face only when read; the same table as a plain dictionary reads the same."""
    from picaso_amd.atmsetup import ATMSETUP, CloudTables
    t, rows, grid, _ = _stub_table()
    case = jdi.inputs()
    case.add_pt(T=np.linspace(500.0, 900.0, 4), P=Z["plevel/3"])
    case.clouds(df=t)
    assert case.inputs["clouds"]["profile"] is t and np.array_equal(case.inputs["clouds"]["wavenumber"], grid)
    assert rows.copies == 0
    wno = np.linspace(40.0, 31000.0, 50)
    atm = ATMSETUP(case.inputs)
    atm.get_profile()
    atm.get_clouds(wno)
    cld = atm.layer["cloud"]
    assert isinstance(cld, CloudTables) and cld.resident is t and not atm.cloud_free and rows.copies == 0
    assert len(cld) == 3 and "opd" in cld and sorted(cld.keys()) == ["g0", "opd", "w0"] and rows.copies == 0
    r3 = rows.rows.reshape(3, 3, 7)
    assert np.array_equal(cld.compact["w0"], r3[1]) and rows.copies == 1
    blk = cld.columns(5, 20)
    assert blk.resident is t and np.array_equal(blk.wno, wno[5:20])
    assert blk.compact is cld.compact and blk.columns(2, 4).compact is cld.compact and rows.copies == 1
    early = ATMSETUP(case.inputs)                      # a block cut before anything was read: still one copy for all blocks
    early.get_profile()
    early.get_clouds(wno)
    cuts = [early.layer["cloud"].columns(0, 25), early.layer["cloud"].columns(25, 50)]
    assert cuts[0].compact is cuts[1].compact is early.layer["cloud"].compact
    plain = jdi.inputs()
    plain.add_pt(T=np.linspace(500.0, 900.0, 4), P=Z["plevel/3"])
    plain.clouds(df=dict(t))
    atm2 = ATMSETUP(plain.inputs)
    atm2.get_profile()
    atm2.get_clouds(wno)
    assert type(atm2.layer["cloud"]) is CloudTables
    for k in ("opd", "w0", "g0"):
        assert np.array_equal(atm2.layer["cloud"].compact[k], cld.compact[k])
        assert np.array_equal(atm2.layer["cloud"][k], cld[k]) and np.array_equal(blk[k], cld[k][:, 5:20])
    wrong = jdi.inputs()
    wrong.add_pt(T=np.linspace(500.0, 900.0, 6), P=Z["plevel/5"])
    with pytest.raises(Exception, match="3 layers in the cloud table"):
        wrong.clouds(df=t)
