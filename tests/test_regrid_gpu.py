"""``spectrum(regrid=...)``: spectra binned to an instrument grid on the device (csrc/regrid.hip, picaso_amd/regrid.py).

The criterion is bit identity throughout, and it is derived, not measured: ``picaso_mean_regrid_dev`` adds a bin's values
in increasing column order to a sum that starts at +0.0 and divides by the count -- the operations, in the order, of
``np.bincount(idx, weights) / counts``, which is what the reference's ``mean_regrid`` evaluates through scipy's
``binned_statistic`` (justplotit.py:31-63) -- and forms the flux ratios with numpy's rounding (no contraction).  Fixture:
tests/golden/regrid.npz, the reference's own output (tests/golden/make_regrid.py)."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_regrid_host import make_regrid

pytestmark = pytest.mark.gpu
DB = os.path.join(GOLDEN, "synthetic_opacities.db")
DB196 = os.path.join(GOLDEN, "synthetic_opacities_196x60.db")
SPECTRAL = ("albedo", "fpfs_reflected", "thermal", "fpfs_thermal", "fpfs_total", "transit_depth")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "regrid.npz"))


@pytest.fixture(scope="module")
def og():
    return np.load(os.path.join(GOLDEN, "optics.npz"))


def _bin(plan, rows):
    """``rows``: [(op, a, b, c, k1, k2)] of host arrays -> (nrows, nbins) through picaso_mean_regrid_dev."""
    from picaso_amd import _lib, regrid
    from picaso_amd.device import DeviceArray
    ctx = _lib.context(0)
    up = lambda a: None if a is None else DeviceArray.from_host(a, ctx)
    spec = [(str(i), op, up(a), up(b), up(c), k1, k2) for i, (op, a, b, c, k1, k2) in enumerate(rows)]
    vals, tails = regrid.Binned(plan, ctx, spec).wait()
    assert tails == []
    return np.stack([vals[str(i)] for i in range(len(rows))])


# ---------------------------------------------------------------------------------------------- 1, 2: the kernel
@pytest.mark.parametrize("name", make_regrid.CASES)
def test_kernel_op0_equals_the_reference_bitwise(gold, name):
    from picaso_amd import justdoit as jdi
    x, y, newx, R = make_regrid.case(name)
    plan = jdi.regrid_plan(x, newx=newx, R=R)
    got = _bin(plan, [(0, y[r], None, None, 0.0, 0.0) for r in range(make_regrid.NROWS)])
    want = gold[name + "/expected"]
    assert got.shape == want.shape
    for r in range(make_regrid.NROWS):
        assert np.array_equal(got[r], want[r], equal_nan=True), (name, r, int(np.sum(~((got[r] == want[r]) | (np.isnan(got[r]) & np.isnan(want[r]))))))


def test_kernel_ops_1_to_3_round_as_numpy_does():
    from picaso_amd import justdoit as jdi
    x, y, newx, R = make_regrid.case("A")
    rng = np.random.default_rng(77)
    n = x.size
    a, a2 = 1e-3 * (0.2 + rng.random(n)), 1e4 * rng.random(n) ** 3
    b = 1e5 * (0.5 + rng.random(n))
    c = 0.1 + 0.4 * rng.random(n)
    k1, k2 = (7.1e9 / 6.9e10) ** 2.0, (7.1e9 / 7.5e12) ** 2.0
    plan = jdi.regrid_plan(x, R=R)
    got = _bin(plan, [(1, c, None, None, k2, 0.0), (2, a2, b, None, k1, 0.0), (3, a2, b, c, k1, k2), (3, a, b, c, k1, k2),
                      (0, y[2], None, None, 0.0, 0.0)])
    fpfs_reflected = c * k2                                         # spectrum.py, _post_reflected
    for i, thermal in ((1, a2), (3, a)):
        fpfs_thermal = thermal / b * k1                             # _post_thermal
        fpfs_total = fpfs_thermal + fpfs_reflected                  # _post_final
        if i == 1:
            assert np.array_equal(got[1], jdi.mean_regrid(x, fpfs_thermal, R=R)[1], equal_nan=True)
            assert np.array_equal(got[2], jdi.mean_regrid(x, fpfs_total, R=R)[1], equal_nan=True)
        else:
            assert np.array_equal(got[3], jdi.mean_regrid(x, fpfs_total, R=R)[1], equal_nan=True)
    assert np.array_equal(got[0], jdi.mean_regrid(x, fpfs_reflected, R=R)[1], equal_nan=True)
    assert np.array_equal(got[4], jdi.mean_regrid(x, y[2], R=R)[1], equal_nan=True)


# ---------------------------------------------------------------------------------------------- 6: the C entry's checks
def test_bad_arguments_are_errors_and_launch_nothing():
    from picaso_amd import _lib, regrid
    from picaso_amd import justdoit as jdi
    from picaso_amd.device import DeviceArray
    lib, ctx = _lib.load(), _lib.context(0)
    x, y, newx, R = make_regrid.case("D")
    plan = jdi.regrid_plan(x, newx=newx)
    d_y, d_start = DeviceArray.from_host(y[0], ctx), plan.device_start(ctx)
    out = DeviceArray.from_host(np.full(2 * plan.nbins, -7.0), ctx)
    good = (regrid._Row * 2)()
    for w in good:
        w.op, w.a = 0, d_y.addr

    def call(ctx_=ctx, nwno=x.size, nbins=plan.nbins, start=d_start.addr, nrows=2, rows=good, out_=out.addr):
        return lib.picaso_mean_regrid_dev(ctx_, ctypes.c_long(nwno), ctypes.c_int(nbins), ctypes.c_void_p(start),
                                          ctypes.c_int(nrows), rows, ctypes.c_void_p(out_))

    def row(op, a=d_y.addr, b=None, c=None):
        r = (regrid._Row * 2)()
        r[0].op, r[0].a = 0, d_y.addr
        r[1].op, r[1].a, r[1].b, r[1].c = op, a, b, c
        return r
    bad = [dict(ctx_=None), dict(start=None), dict(rows=None), dict(out_=None), dict(nbins=0), dict(nbins=-3), dict(nwno=0),
           dict(nrows=0), dict(nrows=regrid.MAX_ROWS + 1), dict(rows=row(4)), dict(rows=row(-1)), dict(rows=row(0, a=None)),
           dict(rows=row(2)), dict(rows=row(3, b=d_y.addr))]
    for kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.picaso_last_error(kw.get("ctx_", ctx))
        assert msg and b"picaso_mean_regrid_dev" in msg, kw
    assert np.array_equal(out.to_host(), np.full(2 * plan.nbins, -7.0))           # nothing was launched
    assert call() == 0
    got = out.to_host().reshape(2, plan.nbins)
    assert np.array_equal(got[0], jdi.mean_regrid(x, y[0], newx=newx)[1]) and np.array_equal(got[1], got[0])


# ---------------------------------------------------------------------------------------------- 3: the product paths
def _star(case, nwno):
    case.star(relative_flux=1.0 + 0.3 * np.sin(np.arange(nwno) / 7.0), radius=6.9e10, semi_major=7.5e12)


def _toon(og, jdi):
    from test_driver_gpu import _case
    return _case(og, jdi, True, True, "none", True), jdi.opannection(filename_db=DB, query_method="linear"), {}


def _toon196(og, jdi):
    g = np.load(os.path.join(GOLDEN, "optics_196x60.npz"))
    opa = jdi.opannection(filename_db=DB196, query_method="linear")
    case = jdi.inputs()
    case.phase_angle(0)
    case.gravity(gravity=float(g["in/gravity"]), radius=7.1e9, mass=1.9e30)
    prof = {"pressure": g["in/plevel_bar"], "temperature": g["in/tlevel"]}
    prof.update({k: g["in/mix/" + k] for k in ("H2", "He", "H2O", "CH4")})
    case.atmosphere(df=prof)
    case.clouds(df={"opd": g["in/cld_opd"], "w0": g["in/cld_w0"], "g0": g["in/cld_g0"]})
    _star(case, opa.nwno)
    case.approx(raman="none", delta_eddington=True)
    case.surface_reflect(0.1)
    return case, opa, {}


def _sh4(og, jdi):
    case, opa, _ = _toon(og, jdi)
    case.approx(raman="none", delta_eddington=True, rt_method="SH", stream=4)
    return case, opa, {}


def _three_d(og, jdi):
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    c = jdi.inputs()
    c.phase_angle(0.7, num_gangle=3, num_tangle=2)
    c.gravity(gravity=float(og["in/gravity"]), radius=7.1e9, mass=1.9e30)
    prof = {"pressure": og["in/plevel_bar"],
            "temperature": og["in/tlevel"][:, None, None] * (1.0 + 0.02 * np.arange(6).reshape(1, 3, 2))}
    for m in ("H2", "He", "H2O", "CH4"):
        prof[m] = og["in/mix/" + m]
    c.atmosphere_3d(prof)
    _star(c, opa.nwno)
    c.approx(raman="none")
    return c, opa, {"dimension": "3d"}


def _transmission(og, jdi):
    case, opa, _ = _toon(og, jdi)
    return case, opa, {"calculation": "reflected+thermal+transmission"}


def _premixed_ck(og, jdi):
    from test_ck_optics import _case, _ck_class
    opa = _ck_class(np.load(os.path.join(GOLDEN, "ck.npz")))
    case = _case(og, jdi)
    case.gravity(gravity=float(og["in/gravity"]), radius=7.1e9, mass=1.9e30)
    _star(case, opa.nwno)
    return case, opa, {}


def _patchy_box_cloud(og, jdi):
    case, opa, _ = _toon(og, jdi)
    nl = len(og["in/plevel_bar"]) - 1
    box = np.zeros((nl, 40))
    box[nl // 3:nl // 3 + 4] = 0.4                                   # a slab of uniform optical depth: the box-cloud form
    case.clouds(df={"opd": box, "w0": np.where(box > 0, 0.95, 0.0), "g0": np.where(box > 0, 0.6, 0.0)},
                wavenumber=np.linspace(opa.wno[0], opa.wno[-1], 40), do_holes=True, fhole=0.3, fthin_cld=0.1)
    return case, opa, {}


def _brown_dwarf(og, jdi):
    from test_driver_gpu import _case
    return _case(og, jdi, False, False, "none", False), jdi.opannection(filename_db=DB, query_method="linear"), \
        {"calculation": "thermal"}


SCENES = {"toon": _toon, "toon196": _toon196, "sh4": _sh4, "3d": _three_d, "transmission": _transmission,
          "premixed_ck": _premixed_ck, "patchy_box_cloud": _patchy_box_cloud, "brown_dwarf": _brown_dwarf}


def _specs(wno):
    """an ``R`` and a ``newx`` plan for the 40- and 196-point grids of the committed databases: bins of one to a few dozen
    points, empty ones, columns outside both ends"""
    lo, hi = float(np.min(wno)), float(np.max(wno))
    newx = np.concatenate([np.linspace(lo + 0.1 * (hi - lo), lo + 0.5 * (hi - lo), 9)[:-1],
                           np.linspace(lo + 0.5 * (hi - lo), lo + 0.55 * (hi - lo), 30),
                           [lo + 0.7 * (hi - lo), lo + 0.85 * (hi - lo)]])
    return {"R": 12}, {"newx": newx}


def _check(jdi, plain, binned, spec, plan):
    assert [k for k in binned if k != "full_output"] == [k for k in plain if k != "full_output"] + ["regrid_counts"]
    x = plain["wavenumber"]
    seen = 0
    for k, v in plain.items():
        if k == "wavenumber":
            assert np.array_equal(binned[k], plan.centres)
        elif k in SPECTRAL and isinstance(v, np.ndarray):
            cx, m = jdi.mean_regrid(x, v, **spec)
            assert np.array_equal(cx, binned["wavenumber"])
            assert binned[k].shape == m.shape and np.array_equal(binned[k], m, equal_nan=True), k
            seen += 1
        elif k == "full_output":
            continue
        else:                                                       # lists, the integrals, the unit string
            assert type(binned[k]) is type(v) and binned[k] == v, k
    assert seen >= 1
    assert np.array_equal(binned["regrid_counts"], plan.counts)
    return seen


@pytest.mark.parametrize("scene", list(SCENES))
def test_product_paths_bin_bit_for_bit(og, scene):
    from picaso_amd import justdoit as jdi
    case, opa, kw = SCENES[scene](og, jdi)
    kw.setdefault("calculation", "reflected+thermal")
    plain = case.spectrum(opa, **kw)
    if scene in ("toon", "toon196", "sh4", "3d"):
        assert opa.__dict__.get("_driver_tables"), "expected the one-C-call driver for this scene"
    arrays = {"toon": 5, "toon196": 5, "sh4": 5, "3d": 5, "transmission": 6, "premixed_ck": 5, "patchy_box_cloud": 5,
              "brown_dwarf": 1}[scene]
    for spec in _specs(opa.wno):
        plan = jdi.regrid_plan(opa, **spec)
        assert plan.counts.max() > 1
        if "newx" in spec:                      # empty bins, and columns outside both ends
            assert plan.counts.min() == 0 and plan.start[0] > 0 and plan.start[-1] < opa.nwno
        for regrid in (spec, plan):
            binned = case.spectrum(opa, regrid=regrid, **kw)
            assert _check(jdi, plain, binned, spec, plan) == arrays
    if scene == "brown_dwarf":
        assert binned["fpfs_thermal"] == ["No star mode for Brown Dwarfs was used"] and "fpfs_total" not in binned
    # the call-by-call path bins the same bits, and full_output stays at native resolution
    # (each against the SAME call without regrid=: full_output writes every plane, and where the bits depend on the plane
    # set -- SH with its cloud-free top, INTEGRATION.md section 3c -- the plain full_output call has them too)
    nod_kw = dict(kw, options=jdi.Options(no_driver=True))
    _check(jdi, case.spectrum(opa, **nod_kw), case.spectrum(opa, regrid=spec, **nod_kw), spec, plan)
    full = case.spectrum(opa, regrid=spec, full_output=True, **kw)
    _check(jdi, case.spectrum(opa, full_output=True, **kw), full, spec, plan)
    assert isinstance(full["full_output"], dict)


def test_no_radii_keeps_the_list_placeholders(og):
    from picaso_amd import justdoit as jdi
    from test_ck_optics import _case
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    case = _case(og, jdi)                                            # gravity alone: NaN radii, no star
    plain = case.spectrum(opa, calculation="reflected+thermal")
    spec = _specs(opa.wno)[0]
    binned = case.spectrum(opa, calculation="reflected+thermal", regrid=spec)
    assert _check(jdi, plain, binned, spec, jdi.regrid_plan(opa, **spec)) == 2
    assert binned["fpfs_reflected"] == [] and "fpfs_total" not in binned


# ---------------------------------------------------------------------------------------------- 4: async and batch
def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


@pytest.mark.parametrize("scene", ["toon", "3d", "transmission", "patchy_box_cloud"])
def test_async_and_batch_equal_the_synchronous_binned_call(og, scene):
    from picaso_amd import justdoit as jdi
    from test_driver_gpu import _case
    case, opa, kw = SCENES[scene](og, jdi)
    kw.setdefault("calculation", "reflected+thermal")
    spec = _specs(opa.wno)[1]
    want = case.spectrum(opa, regrid=spec, **kw)
    pend = [case.spectrum_async(opa, regrid=spec, **kw) for _ in range(jdi.ASYNC_DEPTH + 2)]     # more than the slots
    for p in pend:
        _same(want, p.result())
    if scene == "3d":
        return
    members = [case] + [_case(og, jdi, True, True, "none", True, k) for k in (1, 2)]
    singles = [m.spectrum(opa, regrid=spec, **kw) for m in members]
    _same(want, singles[0])
    outs = jdi.spectrum_batch(members, opa, regrid=spec, batch_size=2, **{k: v for k, v in kw.items() if k != "dimension"})
    for s, o in zip(singles, outs):
        _same(s, o)


# ---------------------------------------------------------------------------------------------- 5: cache, out of scope
def test_equal_R_reuses_one_plan_and_one_upload(og):
    from picaso_amd import justdoit as jdi
    case, opa, _ = _toon(og, jdi)
    a = case.spectrum(opa, calculation="reflected+thermal", regrid={"R": 12})
    plans = opa.__dict__["_regrid_plans"]
    assert len(plans) == 1
    plan = next(iter(plans.values()))
    assert len(plan._dev) == 1
    table = next(iter(plan._dev.values()))
    b = case.spectrum(opa, calculation="reflected+thermal", regrid={"R": 12.0})
    assert len(plans) == 1 and next(iter(plans.values())) is plan and next(iter(plan._dev.values())) is table
    _same(a, b)
    assert jdi.regrid_plan(opa, R=12) is plan


def test_out_of_scope_combinations_say_so(og):
    from picaso_amd import justdoit as jdi
    case, opa, _ = _toon(og, jdi)
    with pytest.raises(NotImplementedError, match="devices"):
        case.spectrum(opa, calculation="reflected", devices=2, regrid={"R": 12})
    with pytest.raises(NotImplementedError, match="phase_curve"):
        case.phase_curve(opa, regrid={"R": 12})
