"""``picaso_instruments_reduce_dev`` (csrc/instruments.hip) through ``regrid.InstrumentsPlan``: several instruments, binned
or convolved each, from one set of resident rows in one call.

Among the device's own results the criterion is bit identity: with ``scale = 1`` a point has the bits of its member plan's
own launch (``picaso_mean_regrid_dev`` / ``picaso_lsf_convolve_dev``).  A mean point is host ``jdi.mean_regrid`` bit for bit,
also with a scale (the column is scaled before it is summed, as the reference scales the flux before it bins).  A Gaussian
point is held to the bound tests/test_convolve_gpu.py holds ``picaso_lsf_convolve_dev`` to against host
``conv_non_uniform_R``, ``(2 n_w + 10) 2^-53 conv(|y|)`` (test_convolve_host.py), plus one unit of ``2^-53`` for the product
where there is a scale.

Shapes: 1 500 columns, three rows (ops 0, 2 and 3, so that ``b`` and ``c`` are read).  A: bins of 0, 1, 63, 64, 65, 128 and
130 columns -- the chunk edges of ``bin_sum``, the empty bin (NaN) and the single column (exact).  B: windows of 0 (NaN), 1,
63, 65, 1 024, 1 025 and 1 400 columns -- around one wave, and around and past one trip of the 1 024 threads.  C: bins that
overlap A's and B's, one of them equal to one of A's."""
import numpy as np
import pytest

from test_convolve_host import bound, within

pytestmark = pytest.mark.gpu

NWNO = 1500
WNO = 1000.0 + np.arange(float(NWNO))
A_NEWX = np.array([999.4, 999.6, 1001.4, 1125.6, 1129.4, 1255.6, 1385.4])
A_COUNTS = [0, 1, 63, 64, 65, 128, 130]
B_WL = np.array([20.0, 1e4 / 1429.0, 5.0, 8.0, 6.0, 5.5, 6.2])
B_R = np.array([1000.0, 48696.8, 1051.7, 632.1, 58.573, 63.085, 35.465])
B_COUNTS = [0, 1, 63, 65, 1024, 1025, 1400]
C_NEWX = np.array([1000.0, 1127.0, 1128.0, 1500.0, 2300.0])
SPEC = {"A": {"newx": A_NEWX}, "B": {"wl": B_WL, "R": B_R}, "C": {"newx": C_NEWX}}
K1, K2 = (7.1e9 / 6.9e10) ** 2.0, (7.1e9 / 7.5e12) ** 2.0
SCALE = 1e-8 * 0.37 ** 2


@pytest.fixture(scope="module")
def vectors():
    rng = np.random.default_rng(1021)
    a = 1e4 * rng.random(NWNO) ** 3 * (1.0 + 0.5 * np.sin(np.arange(NWNO) / 11.0))
    b = 1e5 * (0.5 + rng.random(NWNO))
    c = 0.1 + 0.4 * rng.random(NWNO)
    return a, b, c


def host_rows(vectors):
    """What ``regrid_elem`` forms per column for the three rows, in numpy."""
    a, b, c = vectors
    return [a, a / b * K1, a / b * K1 + c * K2]


def device_rows(vectors):
    a, b, c = vectors
    return [(0, a, None, None, 0.0, 0.0), (2, a, b, None, K1, 0.0), (3, a, b, c, K1, K2)]


def reduce(plan, rows):
    """``rows``: [(op, a, b, c, k1, k2)] of host arrays -> (nrows, nout) through the plan's launch."""
    from picaso_amd import _lib
    from picaso_amd.device import DeviceArray
    ctx = _lib.context(0)
    up = lambda a: None if a is None else DeviceArray.from_host(a, ctx)
    spec = [(str(i), op, up(a), up(b), up(c), k1, k2) for i, (op, a, b, c, k1, k2) in enumerate(rows)]
    vals, tails = plan.enqueue(ctx, spec).wait()
    assert tails == []
    return np.stack([vals[str(i)] for i in range(len(rows))])


@pytest.fixture(scope="module")
def plan():
    from picaso_amd import justdoit as jdi
    p = jdi.instruments_plan(WNO, SPEC)
    assert list(p.members["A"].counts) == A_COUNTS and list(p.members["B"].counts) == B_COUNTS
    a, c = p.members["A"], p.members["C"]
    assert (a.start[3], a.start[4]) == (c.start[1], c.start[2])         # one bin of C is one bin of A
    assert p.nmean == 12 and p.ngauss == 7 and p.nout == 19
    return p


@pytest.fixture(scope="module")
def unscaled(plan, vectors):
    return reduce(plan, device_rows(vectors))


def test_every_point_has_the_bits_of_its_member_plans_own_launch(plan, vectors, unscaled):
    from picaso_amd import justdoit as jdi
    for name, member in plan.members.items():
        own = reduce(member, device_rows(vectors))
        assert np.array_equal(unscaled[:, plan.slices[name]], own, equal_nan=True), name
    for name, newx in (("A", A_NEWX), ("C", C_NEWX)):
        for r, v in enumerate(host_rows(vectors)):
            want = jdi.mean_regrid(WNO, v, newx=newx)[1]
            assert np.array_equal(unscaled[r, plan.slices[name]], want, equal_nan=True), (name, r)
    got = unscaled[:, plan.slices["A"]]
    assert np.all(np.isnan(got[:, 0])) and not np.any(np.isnan(got[:, 1:]))
    assert got[0, 1] == vectors[0][0]                                    # the single column: exact
    assert np.array_equal(unscaled[:, plan.slices["A"]][:, 3], unscaled[:, plan.slices["C"]][:, 1])


def test_gaussian_points_within_the_convolve_bound(plan, vectors, unscaled):
    from picaso_amd import justdoit as jdi
    host = lambda v: jdi.conv_non_uniform_R(v, 1e4 / WNO, B_R, B_WL)
    counts = plan.members["B"].counts
    for r, v in enumerate(host_rows(vectors)):
        got = unscaled[r, plan.slices["B"]]
        print("row", r, "worst |out - ref| / bound:", within(got, host(v), counts, host(np.abs(v))))
        assert list(np.isnan(got)) == [True] + [False] * 6


def test_scale_is_applied_per_column_before_the_sums(plan, vectors):
    from picaso_amd import justdoit as jdi
    a = vectors[0]
    scaled = plan.with_scale(SCALE)
    assert scaled is not plan and scaled.scale == SCALE and plan.scale == 1.0
    got = reduce(scaled, device_rows(vectors)[:1])[0]
    for name, newx in (("A", A_NEWX), ("C", C_NEWX)):
        want = jdi.mean_regrid(WNO, SCALE * a, newx=newx)[1]
        assert np.array_equal(got[plan.slices[name]], want, equal_nan=True), name
    ref = jdi.conv_non_uniform_R(SCALE * a, 1e4 / WNO, B_R, B_WL)
    mag = jdi.conv_non_uniform_R(np.abs(SCALE * a), 1e4 / WNO, B_R, B_WL)
    gb = got[plan.slices["B"]]
    assert np.array_equal(np.isnan(gb), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(gb[ok] - ref[ok])
    lim = (bound(plan.members["B"].counts, mag) + 2.0 ** -53 * mag)[ok]
    print("scaled: worst |out - ref| / bound:", float(np.max(err / lim)))
    assert np.all(err <= lim)


def test_a_point_does_not_depend_on_the_rows_nor_on_the_order_of_the_instruments(plan, vectors, unscaled):
    from picaso_amd import justdoit as jdi
    rows = device_rows(vectors)
    for r in range(3):
        assert np.array_equal(reduce(plan, rows[r:r + 1])[0], unscaled[r], equal_nan=True), r
    other = jdi.instruments_plan(WNO, {k: SPEC[k] for k in ("B", "C", "A")})
    assert list(other.slices) == ["B", "C", "A"] and other.nmean == 12
    got = reduce(other, rows)
    for name in SPEC:
        assert np.array_equal(got[:, other.slices[name]], unscaled[:, plan.slices[name]], equal_nan=True), name


def test_means_alone_need_no_wavelengths_and_gaussians_alone_work(plan, vectors, unscaled):
    from picaso_amd import _lib
    from picaso_amd import justdoit as jdi
    rows = device_rows(vectors)
    means = jdi.instruments_plan(WNO, {"A": SPEC["A"], "C": SPEC["C"]})
    assert means.ngauss == 0 and means.device_tables(_lib.context(0))[2] is None          # wl = NULL
    got = reduce(means, rows)
    assert np.array_equal(got[:, means.slices["A"]], unscaled[:, plan.slices["A"]], equal_nan=True)
    assert np.array_equal(got[:, means.slices["C"]], unscaled[:, plan.slices["C"]], equal_nan=True)
    gauss = jdi.instruments_plan(WNO, {"B": SPEC["B"]})
    assert gauss.nmean == 0
    assert np.array_equal(reduce(gauss, rows), unscaled[:, plan.slices["B"]], equal_nan=True)


def test_bad_arguments_are_errors_and_launch_nothing(plan, vectors, unscaled):
    """Arguments the entry rejects before any launch: non-zero, ``picaso_last_error`` set, ``out`` untouched."""
    from picaso_amd import _lib, regrid
    from picaso_amd.device import DeviceArray
    lib, ctx = _lib.load(), _lib.context(0)
    n = plan.nout
    d_a, d_b = (DeviceArray.from_host(v, ctx) for v in vectors[:2])
    d_int, d_dbl, d_wl = plan.device_tables(ctx)
    out = DeviceArray.from_host(np.full(2 * n, -7.0), ctx)
    good = (regrid._Row * 2)()
    for w in good:
        w.op, w.a = 0, d_a.addr

    def call(ctx_=ctx, nwno=NWNO, wl=d_wl.addr, nmean=plan.nmean, ngauss=plan.ngauss, lo=d_int.addr, hi=d_int.addr + 4 * n,
             col=d_int.addr + 8 * n, centre=d_dbl.addr, den=d_dbl.addr + 8 * n, scale=1.0, nrows=2, rows=good, out_=out.addr):
        return lib.picaso_instruments_reduce_dev(ctx_, nwno, wl, nmean, ngauss, lo, hi, col, centre, den, scale, nrows, rows,
                                                 out_)

    def row(op, a=d_a.addr, b=None, c=None):
        r = (regrid._Row * 2)()
        r[0].op, r[0].a = 0, d_a.addr
        r[1].op, r[1].a, r[1].b, r[1].c = op, a, b, c
        return r
    bad = [dict(ctx_=None), dict(lo=None), dict(hi=None), dict(col=None), dict(centre=None), dict(den=None), dict(rows=None),
           dict(out_=None), dict(wl=None), dict(nmean=0, ngauss=0), dict(nmean=-1), dict(ngauss=-2), dict(nwno=0),
           dict(nwno=2 ** 31), dict(scale=float("nan")), dict(nrows=0), dict(nrows=regrid.MAX_ROWS + 1), dict(rows=row(4)),
           dict(rows=row(-1)), dict(rows=row(0, a=None)), dict(rows=row(2)), dict(rows=row(3, b=d_b.addr))]
    for kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.picaso_last_error(kw.get("ctx_", ctx))
        assert msg and b"picaso_instruments_reduce_dev" in msg, kw
    assert np.array_equal(out.to_host(), np.full(2 * n, -7.0))                    # nothing was launched
    assert call() == 0                                                            # ... and a valid call still works
    got = out.to_host().reshape(2, n)
    assert np.array_equal(got[0], unscaled[0], equal_nan=True) and np.array_equal(got[1], got[0], equal_nan=True)
    assert call(wl=None, ngauss=0, nrows=1) == 0                                  # no Gaussian points: wl may be NULL
