"""``spectrum(convolve=...)``: spectra convolved with a line-spread function on the device (csrc/convolve.hip,
picaso_amd/convolve.py).  Fixture: tests/golden/convolve.npz, the reference's own ``conv_non_uniform_R``
(tests/golden/make_convolve.py).

The tolerance is derived in test_convolve_host.py: ``|out - ref| <= (2 n_w + 10) 2^-53 conv(|y|)`` per point, ``n_w`` the
point's own count of columns -- the kernel's argument of ``exp`` has numpy's bits, so only ``exp``'s rounding and the order
of the two sums differ.  Among the device's own results the criterion is bit identity: a point's sums are taken in an order
that depends on its window alone."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_convolve_host import bound, make_convolve, within          # noqa: F401

pytestmark = pytest.mark.gpu
DB = os.path.join(GOLDEN, "synthetic_opacities.db")
DB196 = os.path.join(GOLDEN, "synthetic_opacities_196x60.db")
SPECTRAL = ("albedo", "fpfs_reflected", "thermal", "fpfs_thermal", "fpfs_total", "transit_depth")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "convolve.npz"))


@pytest.fixture(scope="module")
def og():
    return np.load(os.path.join(GOLDEN, "optics.npz"))


def _convolve(plan, rows):
    """``rows``: [(op, a, b, c, k1, k2)] of host arrays -> (nrows, nobs) through picaso_lsf_convolve_dev."""
    from picaso_amd import _lib
    from picaso_amd.device import DeviceArray
    ctx = _lib.context(0)
    up = lambda a: None if a is None else DeviceArray.from_host(a, ctx)
    spec = [(str(i), op, up(a), up(b), up(c), k1, k2) for i, (op, a, b, c, k1, k2) in enumerate(rows)]
    vals, tails = plan.enqueue(ctx, spec).wait()
    assert tails == []
    return np.stack([vals[str(i)] for i in range(len(rows))])


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", make_convolve.CASES)
def test_kernel_against_the_reference_within_the_bound(gold, name):
    from picaso_amd import justdoit as jdi
    x, y, wl, R = make_convolve.case(name)
    plan = jdi.convolve_plan(x, wl, R)
    got = _convolve(plan, [(0, y[r], None, None, 0.0, 0.0) for r in range(2)])
    want, scale = gold[name + "/expected"], gold[name + "/expected_abs"]
    assert got.shape == want.shape
    for r in range(2):
        print(name, r, "worst |out - ref| / bound:", within(got[r], want[r], plan.counts, scale[r]))
    if name == "D":
        assert list(np.isnan(got[0])) == [True, False, False, False, True]
    if name == "E":
        assert list(np.isnan(got[0])) == [True] + [False] * 5


def test_kernel_ops_1_to_3_against_the_host_function():
    from picaso_amd import justdoit as jdi
    x, y, wl, R = make_convolve.case("A")
    rng = np.random.default_rng(77)
    n = x.size
    a, a2 = 1e-3 * (0.2 + rng.random(n)), 1e4 * rng.random(n) ** 3
    b = 1e5 * (0.5 + rng.random(n))
    c = 0.1 + 0.4 * rng.random(n)
    k1, k2 = (7.1e9 / 6.9e10) ** 2.0, (7.1e9 / 7.5e12) ** 2.0
    plan = jdi.convolve_plan(x, wl, R)
    got = _convolve(plan, [(1, c, None, None, k2, 0.0), (2, a2, b, None, k1, 0.0), (3, a2, b, c, k1, k2), (3, a, b, c, k1, k2),
                           (0, y[1], None, None, 0.0, 0.0)])
    fpfs_reflected = c * k2                                         # spectrum.py, _post_reflected
    host = lambda v: jdi.conv_non_uniform_R(v, 1e4 / x, R, wl)
    want = [fpfs_reflected, a2 / b * k1, a2 / b * k1 + fpfs_reflected, a / b * k1 + fpfs_reflected, y[1]]
    for i, v in enumerate(want):
        within(got[i], host(v), plan.counts, host(np.abs(v)))


def test_bad_arguments_are_errors_and_launch_nothing(gold):
    from picaso_amd import _lib, regrid
    from picaso_amd import justdoit as jdi
    from picaso_amd.device import DeviceArray
    lib, ctx = _lib.load(), _lib.context(0)
    x, y, wl, R = make_convolve.case("E")
    plan = jdi.convolve_plan(x, wl, R)
    nobs = plan.nobs
    d_y = DeviceArray.from_host(y[0], ctx)
    d_wl, d_c, d_den, d_win = plan.device_tables(ctx)
    out = DeviceArray.from_host(np.full(2 * nobs, -7.0), ctx)
    good = (regrid._Row * 2)()
    for w in good:
        w.op, w.a = 0, d_y.addr

    def call(ctx_=ctx, nwno=x.size, wl_=d_wl.addr, nobs_=nobs, centre=d_c.addr, den=d_den.addr, lo=d_win.addr,
             hi=d_win.addr + 4 * nobs, nrows=2, rows=good, out_=out.addr):
        return lib.picaso_lsf_convolve_dev(ctx_, ctypes.c_long(nwno), ctypes.c_void_p(wl_), ctypes.c_int(nobs_),
                                           ctypes.c_void_p(centre), ctypes.c_void_p(den), ctypes.c_void_p(lo),
                                           ctypes.c_void_p(hi), ctypes.c_int(nrows), rows, ctypes.c_void_p(out_))

    def row(op, a=d_y.addr, b=None, c=None):
        r = (regrid._Row * 2)()
        r[0].op, r[0].a = 0, d_y.addr
        r[1].op, r[1].a, r[1].b, r[1].c = op, a, b, c
        return r
    bad = [dict(ctx_=None), dict(wl_=None), dict(centre=None), dict(den=None), dict(lo=None), dict(hi=None), dict(rows=None),
           dict(out_=None), dict(nobs_=0), dict(nobs_=-3), dict(nwno=0), dict(nrows=0), dict(nrows=regrid.MAX_ROWS + 1),
           dict(rows=row(4)), dict(rows=row(-1)), dict(rows=row(0, a=None)), dict(rows=row(2)), dict(rows=row(3, b=d_y.addr))]
    for kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.picaso_last_error(kw.get("ctx_", ctx))
        assert msg and b"picaso_lsf_convolve_dev" in msg, kw
    assert np.array_equal(out.to_host(), np.full(2 * nobs, -7.0))                 # nothing was launched
    assert call() == 0                                                            # ... and a valid call still works
    got = out.to_host().reshape(2, nobs)
    within(got[0], gold["E/expected"][0], plan.counts, gold["E/expected_abs"][0])
    assert np.array_equal(got[1], got[0], equal_nan=True)


def test_a_points_bits_depend_on_its_window_alone():
    from picaso_amd import justdoit as jdi
    x, y, wl, R = make_convolve.case("A")
    plan = jdi.convolve_plan(x, wl, R)
    rows = [(0, y[0], None, None, 0.0, 0.0), (0, y[1], None, None, 0.0, 0.0)]
    first, second = _convolve(plan, rows), _convolve(plan, rows)
    assert np.array_equal(first, second)
    # the same rows among more rows, the same points among more points (in front of them, between them, behind them)
    more_wl = np.concatenate([[0.5, 3.3], wl[:20], [1.234], wl[20:], np.linspace(0.4, 4.0, 300)])
    more_R = np.concatenate([[40.0, 900.0], R[:20], [250.0], R[20:], np.linspace(30.0, 300.0, 300)])
    where = np.concatenate([2 + np.arange(20), 23 + np.arange(17)])
    big = jdi.convolve_plan(x, more_wl, more_R)
    assert np.array_equal(big.counts[where], plan.counts)
    b = 0.5 + np.abs(y[1])
    got = _convolve(big, [(2, y[1], b, None, 3.0, 0.0), rows[0], (1, y[0], None, None, 0.3, 0.0), (3, y[0], b, y[1], 2.0, 5.0),
                          rows[1], (0, b, None, None, 0.0, 0.0)])
    assert np.array_equal(got[1][where], first[0]) and np.array_equal(got[4][where], first[1])


# ---------------------------------------------------------------------------------------------- the product paths
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


def _brown_dwarf(og, jdi):
    from test_driver_gpu import _case
    return _case(og, jdi, False, False, "none", False), jdi.opannection(filename_db=DB, query_method="linear"), \
        {"calculation": "thermal"}


SCENES = {"toon196": _toon196, "sh4": _sh4, "3d": _three_d, "transmission": _transmission, "brown_dwarf": _brown_dwarf}


def _spec():
    """data on the 0.4-2.5 um grids of the committed databases: descending wavelengths, one given twice, R rising from 6
    to 25 (windows of a few columns to most of the grid), and one point far outside the grid (NaN)"""
    wl = np.array([2.3, 2.05, 1.8, 1.55, 1.3, 1.8, 1.05, 0.8, 0.62, 0.45, 9.0])
    R = np.array([6.0, 8.0, 10.0, 12.0, 14.0, 10.0, 16.0, 18.0, 20.0, 25.0, 60.0])
    return {"wl": wl, "R": R}


def _check(jdi, plain, conv, spec, plan):
    assert [k for k in conv if k != "full_output"] == [k for k in plain if k != "full_output"] + ["convolve_counts"]
    model_wl = 1e4 / plain["wavenumber"]
    seen = 0
    for k, v in plain.items():
        if k == "wavenumber":
            assert np.array_equal(conv[k], 1e4 / spec["wl"])
        elif k in SPECTRAL and isinstance(v, np.ndarray):
            want = jdi.conv_non_uniform_R(v, model_wl, spec["R"], spec["wl"])
            scale = jdi.conv_non_uniform_R(np.abs(v), model_wl, spec["R"], spec["wl"])
            assert np.isnan(want[-1]) and not np.any(np.isnan(want[:-1]))
            within(conv[k], want, plan.counts, scale)
            assert conv[k][5] == conv[k][2]                          # the point given twice
            seen += 1
        elif k == "full_output":
            continue
        else:                                                       # lists, the integrals, the unit string
            assert type(conv[k]) is type(v) and conv[k] == v, k
    assert seen >= 1
    assert np.array_equal(conv["convolve_counts"], plan.counts)
    return seen


@pytest.mark.parametrize("scene", list(SCENES))
def test_product_paths_convolve_within_the_bound(og, scene):
    from picaso_amd import justdoit as jdi
    case, opa, kw = SCENES[scene](og, jdi)
    kw.setdefault("calculation", "reflected+thermal")
    plain = case.spectrum(opa, **kw)
    if scene in ("toon196", "sh4", "3d"):
        assert opa.__dict__.get("_driver_tables"), "expected the one-C-call driver for this scene"
    arrays = {"toon196": 5, "sh4": 5, "3d": 5, "transmission": 6, "brown_dwarf": 1}[scene]
    spec = _spec()
    plan = jdi.convolve_plan(opa, **spec)
    assert plan.counts[-1] == 0 and plan.counts[:-1].min() >= 1 and plan.counts.max() > opa.nwno // 2
    by_dict = case.spectrum(opa, convolve=spec, **kw)
    assert _check(jdi, plain, by_dict, spec, plan) == arrays
    _same(by_dict, case.spectrum(opa, convolve=plan, **kw))
    if scene == "brown_dwarf":
        assert by_dict["fpfs_thermal"] == ["No star mode for Brown Dwarfs was used"] and "fpfs_total" not in by_dict
    # the call-by-call path convolves within the same bound, and full_output stays at native resolution (each against the
    # SAME call without convolve=, as tests/test_regrid_gpu.py explains)
    nod_kw = dict(kw, options=jdi.Options(no_driver=True))
    _check(jdi, case.spectrum(opa, **nod_kw), case.spectrum(opa, convolve=spec, **nod_kw), spec, plan)
    full = case.spectrum(opa, convolve=spec, full_output=True, **kw)
    _check(jdi, case.spectrum(opa, full_output=True, **kw), full, spec, plan)
    assert isinstance(full["full_output"], dict)
    assert len(opa.__dict__["_convolve_plans"]) == 1 and len(plan._dev) >= 1      # one plan, found by content


# ---------------------------------------------------------------------------------------------- async and batch
def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


@pytest.mark.parametrize("scene", ["toon", "3d", "transmission"])
def test_async_and_batch_equal_the_synchronous_convolved_call(og, scene):
    from picaso_amd import justdoit as jdi
    from test_driver_gpu import _case
    case, opa, kw = dict(SCENES, toon=_toon)[scene](og, jdi)
    kw.setdefault("calculation", "reflected+thermal")
    spec = _spec()
    want = case.spectrum(opa, convolve=spec, **kw)
    assert "convolve_counts" in want and want["albedo"].shape == (11,)
    pend = [case.spectrum_async(opa, convolve=spec, **kw) for _ in range(jdi.ASYNC_DEPTH + 2)]     # more than the slots
    for p in pend:
        _same(want, p.result())
    if scene == "3d":
        return
    members = [case] + [_case(og, jdi, True, True, "none", True, k) for k in (1, 2)]
    singles = [m.spectrum(opa, convolve=spec, **kw) for m in members]
    _same(want, singles[0])
    outs = jdi.spectrum_batch(members, opa, convolve=spec, batch_size=2, **{k: v for k, v in kw.items() if k != "dimension"})
    for s, o in zip(singles, outs):
        _same(s, o)


# ---------------------------------------------------------------------------------------------- errors
def test_out_of_scope_combinations_say_so(og):
    from picaso_amd import justdoit as jdi
    case, opa, _ = _toon(og, jdi)
    spec = _spec()
    with pytest.raises(Exception, match="give one of them"):
        case.spectrum(opa, calculation="reflected", regrid={"R": 12}, convolve=spec)
    with pytest.raises(Exception, match="give one of them"):
        case.spectrum_async(opa, calculation="reflected", regrid={"R": 12}, convolve=spec)
    with pytest.raises(NotImplementedError, match="devices"):
        case.spectrum(opa, calculation="reflected", devices=2, convolve=spec)
    with pytest.raises(NotImplementedError, match="phase_curve"):
        case.phase_curve(opa, convolve=spec)
    other = jdi.opannection(filename_db=DB196, query_method="linear")
    with pytest.raises(Exception, match="another wavenumber grid"):
        case.spectrum(opa, calculation="reflected", convolve=jdi.convolve_plan(other, **spec))
    with pytest.raises(Exception, match="R must be positive"):
        case.spectrum(opa, calculation="reflected", convolve={"wl": spec["wl"], "R": 0.0})
    with pytest.raises(Exception, match="different lengths"):
        case.spectrum(opa, calculation="reflected", convolve={"wl": spec["wl"], "R": spec["R"][:4]})
    # ... and the case still runs
    assert case.spectrum(opa, calculation="reflected", convolve=spec)["albedo"].shape == (11,)
