"""``picaso_mie_q_dev`` (csrc/mie.hip), ``picaso_mie_cloud_tables_dev`` (csrc/miecloud.hip) and their Python faces in
``picaso_amd.mie`` on the GPU: the device series against 40-digit mpmath, the shapes at which the kernel's packing into
waves and chunks can go wrong, the table maker against the host mean, the batch of cloud tables against the host functions
bit for bit, and spectra fed from the batch against the same spectra fed the host DataFrames."""
import numpy as np
import pytest

from mie_cases import U, case_list, errors, synthetic_table
from test_devices_gpu import _same
from test_parameterize_gpu import _case, og, opa  # noqa: F401  (og, opa: fixtures)

pytestmark = pytest.mark.gpu


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _param(nlayer):
    from picaso_amd import justdoit as jdi
    from picaso_amd import parameterizations as pz
    case = jdi.inputs()
    case.add_pt(P=np.logspace(-5.5, 1.7, nlayer + 1))
    p = pz.Parameterize()
    p.add_class(case)
    return p


# ---- the series
def test_device_series_against_mpmath():
    """Every case of the list within 8 x the worst error of ``mie_efficiencies_numpy`` against mpmath on the same list
    (never below 64 x 2^-53), in the three measures.  The factor covers the device's sin / cos and up to ~3e3 accumulated
    terms; the device forms its complex quotients as numpy does.  Measured on an MI355X (worst of the list, Qext / Qsca /
    g): numpy 9.46e-15 / 1.30e-14 / 1.17e-14, device 9.46e-15 / 1.30e-14 / 1.19e-14, allowed 1.04e-13."""
    from picaso_amd import mie
    x, m = case_list()
    host = errors(mie.mie_efficiencies_numpy(x, m))
    got = errors(mie.mie_efficiencies(x, m))
    tol = max(8.0 * host.max(), 64.0 * U)
    print("worst error against mpmath (Qext, Qsca, g): numpy %.3g %.3g %.3g, device %.3g %.3g %.3g, allowed %.3g"
          % (tuple(host.max(axis=1)) + tuple(got.max(axis=1)) + (tol,)))
    assert got.shape == (3, 64) and np.all(got <= tol), (got.max(axis=1), np.argmax(got, axis=1), tol)


def _mixed(n, seed=8):
    """``n`` elements whose neighbours are far apart: x = 1e-6 (nstop = 2) next to x = 1e3, then everything between."""
    rng = np.random.default_rng(seed)
    x = 10 ** rng.uniform(-6, 3, n)
    x[0::7], x[1::7] = 1e-6, 1e3
    k = 10 ** rng.uniform(-8, 0.4, n)
    k[::5] = 0
    return x[:n], (rng.uniform(1.05, 3, n) + 1j * k)[:n]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_lengths_around_a_wave(n):
    """One element, one short of a wave, a wave, one over, and three waves and a part: against the numpy series at the
    device's tolerance against mpmath (the list's largest x is 1e3, as there), the NaNs where numpy has them."""
    from picaso_amd import mie
    x, m = _mixed(n)
    got, want = mie.mie_efficiencies(x, m), mie.mie_efficiencies_numpy(x, m)
    assert all(g.shape == (n,) and np.all(np.isfinite(g)) for g in got)
    tol = 64.0 * U + 8.0 * 1.3e-14
    assert np.all(np.abs(got[0] - want[0]) <= tol * want[0]) and np.all(np.abs(got[1] - want[1]) <= tol * want[1])
    assert np.all(np.abs(got[2] - want[2]) <= tol * want[1])


def test_chunks_wave_mates_and_refused_elements():
    """200 unsorted elements with x = 1e-6 and x = 1e3 as neighbours, NaN, x = 0 and k < 0 among them: the result of one
    chunk, of at least three chunks and of five elements passed alone are the same bits, in any shape."""
    from picaso_amd import mie
    x, m = _mixed(200)
    x[3], x[64], m[130] = np.nan, 0.0, 1.5 - 1e-3j
    bad = np.zeros(200, dtype=bool)
    bad[[3, 64, 130]] = True
    before = mie.MIE_LAUNCHES
    one = mie.mie_efficiencies(x, m)
    assert mie.MIE_LAUNCHES == before + 1
    # 8 KB: the wave of the largest x (1.6 MB of terms) and the next (14 KB) each exceed it alone, the last two share it
    many = mie.mie_efficiencies(x, m, _scratch_bytes=8 << 10)
    assert mie.MIE_LAUNCHES == before + 1 + 3
    for a, b in zip(one, many):
        assert _bits(a, b) and np.array_equal(np.isnan(a), bad)
    for i in (0, 1, 2, 77, 199):
        alone = mie.mie_efficiencies(x[i], m[i])
        assert all(a.shape == () and _bits(a, b[i]) for a, b in zip(alone, one)), i
    grid = mie.mie_efficiencies(x.reshape(8, 25), m.reshape(8, 25))
    assert all(g.shape == (8, 25) and _bits(g.reshape(-1), a) for g, a in zip(grid, one))
    assert all(g.shape == (0,) for g in mie.mie_efficiencies(np.zeros(0), 1.5))


def test_a_series_over_the_cap_is_a_clean_error():
    from picaso_amd import _lib, mie
    x, m = _mixed(70)
    x[11] = 2.0e6
    with pytest.raises(_lib.PicasoHipError, match="picaso_mie_q_dev.*at most 1048576"):
        mie.mie_efficiencies(x, m)
    with pytest.raises(_lib.PicasoHipError, match="picaso_mie_q_dev"):
        mie.mie_efficiencies(np.inf, 1.5)
    got = mie.mie_efficiencies(2 * np.pi * 0.525 / 0.6328, 1.55)       # the context goes on
    assert abs(float(got[0]) - 3.1054255314658774) <= 1e-12


def test_the_c_entry_of_the_series_refuses_bad_arguments():
    from picaso_amd import _lib
    from picaso_amd.device import DeviceArray
    ctx, lib = _lib.context(), _lib.load()
    x, mre, mim = np.array([1.0, 2.0]), np.array([1.5, 1.5]), np.zeros(2)
    nstop, nmx = np.array([7, 9], dtype=np.int32), np.array([24, 27], dtype=np.int32)
    mark = np.full((3, 2), -7.0)
    out, scratch = DeviceArray.from_host(mark, ctx), DeviceArray((9 * 3 * 64,), ctx)

    def call(n=2, nstop=nstop, nmx=nmx, scratch_bytes=scratch.nbytes, **null):
        args = dict(x=x, m_re=mre, m_im=mim, nstop=nstop, nmx=nmx, scratch=scratch, out=out)
        args.update(null)
        rc = lib.picaso_mie_q_dev(ctx, n, *[_lib.addr(args[k]) for k in ("x", "m_re", "m_im", "nstop", "nmx", "scratch")],
                                  scratch_bytes, _lib.addr(args["out"]))
        return rc, out.to_host()

    i32 = lambda *v: np.array(v, dtype=np.int32)
    for kw in (dict(n=0), dict(x=None), dict(nmx=None), dict(out=None), dict(scratch=None), dict(scratch_bytes=9 * 3 * 64 * 8 - 8),
               dict(nstop=i32(7, 27)), dict(nstop=i32(-1, 9)), dict(nmx=i32(24, (1 << 20) + 1)), dict(nstop=i32(7, 9), nmx=i32(24, 0))):
        rc, rows = call(**kw)
        assert rc != 0 and np.array_equal(rows, mark), kw
        assert b"picaso_mie_q_dev" in lib.picaso_last_error(ctx), kw
    assert lib.picaso_mie_q_dev(None, 2, None, None, None, None, None, None, 0, None) != 0
    rc, rows = call()
    assert rc == 0 and np.all(rows > 0)
    rc, rows = call(nstop=i32(0, 9), nmx=i32(0, 27))                   # marked as not evaluated: NaN, the other as before
    assert rc == 0 and np.all(np.isnan(rows[:, 0])) and np.all(rows[:, 1] > 0)


# ---- the table maker
@pytest.mark.parametrize("nsub", [6, 1])
def test_compute_mieff_is_the_host_mean_of_the_device_series(nsub):
    from picaso_amd import mie
    wave, radius = np.array([0.6, 1.0, 2.5, 5.0, 11.0]), np.array([1e-5, 4e-5, 2e-4])
    nn, kk = np.linspace(1.4, 1.7, 5), np.array([0.0, 1e-4, 1e-2, 0.1, 0.5])
    before = mie.MIE_LAUNCHES
    t = mie.compute_mieff(wave, nn, kk, radius, nsub=nsub)
    assert mie.MIE_LAUNCHES == before + 1 and t.qext.shape == (5, 3) and _bits(t.wave_in[:, 0], wave[::-1])
    sub = mie.sub_radii(radius, None, nsub)
    q = mie.mie_efficiencies(2 * mie.PI * sub[None, :, :] / (wave * 1e-4)[:, None, None], (nn + 1j * kk)[:, None, None])
    for got, each in zip((t.qext, t.qscat, t.cos_qscat), q):
        acc = each[:, :, 0]
        for j in range(1, nsub):
            acc = acc + each[:, :, j]
        assert _bits(got, (acc / nsub)[::-1])
    host = mie.compute_mieff(wave, nn, kk, radius, nsub=nsub, efficiencies=mie.mie_efficiencies_numpy)
    assert np.allclose(t.qext, host.qext, rtol=1e-12, atol=0) and np.allclose(t.cos_qscat, host.cos_qscat, rtol=1e-11, atol=1e-30)


# ---- the batch of cloud tables
LOGNORM = {"sigma": 0.45, "lograd": -3.9}
HANSEN = {"b": 0.17, "lograd": -3.5}


def _decks(p, ta, tb, k):
    """Sample ``k``: a Brewster deck on table ``ta`` and a flex_fsed deck on table ``tb``, parameters moving with ``k``."""
    pl = p.pressure_layer
    lo, hi = np.log10(pl[0]), np.log10(pl[-1])
    if p.nlayer >= 4:
        brew = dict(kind="brewster_mie", table=ta, distribution="hansen", decay_type="slab",
                    hansen_kwargs={"b": 0.17 + 0.02 * k, "lograd": -3.5 - 0.1 * k},
                    slab_kwargs=dict(ptop=lo + 0.25 * (hi - lo), dp=0.4 * (hi - lo), reference_tau=0.5 + 0.3 * k))
    else:
        brew = dict(kind="brewster_mie", table=ta, distribution="lognorm", decay_type="deck",
                    lognorm_kwargs={"sigma": 0.45 + 0.05 * k, "lograd": -3.9}, deck_kwargs=dict(ptop=hi - 1.5, dp=0.5))
    flex = dict(kind="flex_fsed", table=tb, distribution="lognorm", base_pressure=float(pl[(2 * p.nlayer) // 3]) * 1.001,
                ndz=2.5e7 * (1 + k), fsed=0.7 + 0.5 * k, lognorm_kwargs={"sigma": 0.3 + 0.1 * k, "lograd": -4.1 + 0.2 * k})
    return brew, flex


def _host_rows(p, sample, average):
    """The same sample through the host functions (and ``cloud_averaging``): ``(3, nlayer, nwave)``."""
    from picaso_amd import mie
    from picaso_amd import parameterizations as pz
    dfs = []
    for deck in sample:
        kw = {k: v for k, v in deck.items() if k != "kind"}
        dfs.append((mie.cloud_brewster_mie if deck["kind"] == "brewster_mie" else mie.cloud_flex_fsed)(p, **kw))
    df = pz.cloud_averaging(dfs) if average else dfs[0]
    return np.array([df[k].values for k in ("opd", "w0", "g0")]).reshape(3, p.nlayer, -1)


def _check(p, samples, average=None, members=None):
    from picaso_amd import mie
    from picaso_amd import parameterizations as pz
    before = mie.LAUNCHES
    tabs = mie.cloud_tables_batch(p, samples, average=average)
    assert mie.LAUNCHES == before + 1 and len(tabs) == len(samples) and all(isinstance(t, pz.ParamCloudTable) for t in tabs)
    avg = int(max(len(s) for s in samples) > 1) if average is None else average
    rows = []
    for s in (range(len(samples)) if members is None else members):
        got = tabs[s].d_stack.to_host().reshape(3, p.nlayer, -1)
        want = _host_rows(p, samples[s], avg)
        for j, name in enumerate(("opd", "w0", "g0")):
            assert _bits(got[j], want[j]), (s, name, np.max(np.abs(got[j] - want[j])))
        rows.append(got)
    return tabs, rows


@pytest.mark.parametrize("nlayer,nwave,ra,rb,S", [(1, 2, 1, 1, 1), (5, 196, 60, 1, 3), (33, 600, 60, 60, 3)])
def test_cloud_tables_batch_is_the_host_route(nlayer, nwave, ra, rb, S):
    """One launch against ``cloud_brewster_mie`` / ``cloud_flex_fsed`` (and ``cloud_averaging``) per sample, bit for bit:
    one deck of either kind stored as it is and through the averaging, two decks of mixed kinds on two tables, a sample with
    fewer decks than the longest, and a deck whose base lies above every layer (all zero, 1e-33 after the averaging).
    600 wavelengths are three tiles of 256."""
    p = _param(nlayer)
    ta, tb = synthetic_table(nwave, ra, seed=3), synthetic_table(nwave, rb, seed=4)
    pairs = [_decks(p, ta, tb, k) for k in range(S)]
    _, rows = _check(p, [[b] for b, _ in pairs], average=0)
    assert all(np.any(r[0] > 0) and np.all(np.isfinite(r)) for r in rows)
    _, rows = _check(p, [[f] for _, f in pairs], average=0)
    assert all(np.any(r[0] > 0) and (nlayer == 1 or not np.any(r[0][-1])) for r in rows)      # nothing below the base
    _check(p, [[b] for b, _ in pairs], average=1)
    mixed = [list(pair) for pair in pairs]
    if S > 1:
        mixed[1] = mixed[1][1:]                         # fewer decks than the longest
        mixed[2] = mixed[2][::-1]                       # the kinds the other way round
    _, rows = _check(p, mixed)
    assert all(np.all(r[0] > 0) for r in rows)
    none = dict(pairs[0][1], base_pressure=float(p.pressure_layer[0]) * 0.5)
    _, rows = _check(p, [[none]], average=0)
    assert not np.any(rows[0])
    _, rows = _check(p, [[none]] + [[none, none]] * (S - 1), average=1)
    assert all(np.all(r[0] == 1e-33) and not np.any(r[1:]) for r in rows)


def test_many_samples_take_several_layers_per_workgroup():
    """S x tiles x nlayer = 70 x 1 x 33 is past the 2048 at which a workgroup takes two layers and not one: five members
    against the host route, and the first against the same sample launched alone."""
    from picaso_amd import mie
    p = _param(33)
    ta, tb = synthetic_table(2, 60, seed=3), synthetic_table(2, 1, seed=4)
    samples = [list(_decks(p, ta, tb, k % 7)) for k in range(70)]
    tabs, rows = _check(p, samples, members=(0, 1, 34, 68, 69))
    alone = mie.cloud_tables_batch(p, samples[:1])[0]
    assert _bits(alone.d_stack.to_host(), tabs[0].d_stack.to_host())
    assert len({t.d_stack.addr for t in tabs}) == 70 and all(t.d_stack._owner is tabs[0].d_stack._owner for t in tabs)


def test_tables_are_uploaded_once_and_bad_batches_are_refused():
    from picaso_amd import _lib, mie
    from picaso_amd.device import DeviceArray
    p = _param(5)
    ta, tb = synthetic_table(7, 4, seed=3), synthetic_table(7, 1, seed=4)
    sample = list(_decks(p, ta, tb, 0))
    mie.cloud_tables_batch(p, [sample])
    before = mie.TABLE_UPLOADS
    mie.cloud_tables_batch(p, [sample, sample])
    mie.cloud_tables_batch(p, [[dict(sample[0], table=synthetic_table(7, 4, seed=3))]])     # the same content, another object
    assert mie.TABLE_UPLOADS == before
    assert mie.cloud_tables_batch(p, []) == []
    with pytest.raises(ValueError, match="average=0"):
        mie.cloud_tables_batch(p, [sample], average=0)
    ctx, lib = _lib.context(), _lib.load()
    d_t = ta.resident(ctx)
    mark = np.full((1, 3, 5, 7), -7.0)
    out = DeviceArray.from_host(mark, ctx)
    dev = [DeviceArray.zeros(s, ctx) for s in ((1, 1, 4), (1, 1, 5), (1, 1, 5), (1 * (3 * 7 + 1),))]
    i32 = lambda *v: np.array(v, dtype=np.int32)

    def call(S=1, K=1, nlayer=5, nwave=7, average=0, ntable=1, nradii=i32(4), deck_table=i32(0), deck_kind=i32(0), rmax=4, null=None):
        ptrs = [_lib.ptr_array([d_t]), _lib.addr(nradii), _lib.addr(deck_table), _lib.addr(deck_kind)]
        tail = [d.addr for d in dev] + [out.addr]
        if null is not None:
            (ptrs if null < 4 else tail)[null % 4 if null < 4 else null - 4] = None
        rc = lib.picaso_mie_cloud_tables_dev(ctx, S, K, nlayer, nwave, average, ntable, *ptrs, rmax, *tail)
        return rc, out.to_host()

    for kw in (dict(S=0), dict(K=0), dict(K=5), dict(nlayer=0), dict(nwave=1), dict(average=2), dict(ntable=0), dict(rmax=0),
               dict(nradii=i32(5)), dict(nradii=i32(0)), dict(deck_table=i32(1)), dict(deck_table=i32(-2)),
               dict(deck_table=i32(-1)), dict(deck_kind=i32(2)), dict(K=2), dict(null=0), dict(null=3), dict(null=4), dict(null=8)):
        rc, rows = call(**kw)
        assert rc != 0 and np.array_equal(rows, mark), kw
        assert b"picaso_mie_cloud_tables_dev" in lib.picaso_last_error(ctx), kw
    rc, rows = call()
    assert rc == 0 and not np.any(rows == -7.0)


# ---- end to end
def test_spectrum_batch_from_the_batch_tables(og, opa):
    """Three samples through ``spectrum_batch`` (reflected + thermal) fed the tables made in HBM against the same cases fed
    the host DataFrames: bit for bit, and no cloud upload for the tables made in HBM."""
    from picaso_amd import justdoit as jdi
    from picaso_amd import mie, optics
    from picaso_amd import parameterizations as pz
    wno = og["in/wno"]
    lo_um, hi_um = 1e4 / (wno.max() * 0.97), 1e4 / (wno.min() * 1.02)
    ta = synthetic_table(67, 60, seed=3, lo_um=lo_um, hi_um=hi_um)
    tb = synthetic_table(67, 1, seed=4, lo_um=lo_um, hi_um=hi_um)
    p = pz.Parameterize()
    p.add_class(_case(og))
    samples = []
    for k in range(3):
        brew, flex = _decks(p, ta, tb, k)
        samples.append([brew, dict(flex, ndz=3e5 * (1 + k))])
    tabs = mie.cloud_tables_batch(p, samples)
    before = optics.CLOUD_UPLOADS
    got = jdi.spectrum_batch([_case(og, t, k) for k, t in enumerate(tabs)], opa, calculation="reflected+thermal")
    assert optics.CLOUD_UPLOADS == before and not any(t.materialized for t in tabs)
    frames = []
    for sample in samples:
        kws = [{k: v for k, v in d.items() if k != "kind"} for d in sample]
        frames.append(pz.cloud_averaging([mie.cloud_brewster_mie(p, **kws[0]), mie.cloud_flex_fsed(p, **kws[1])]))
    want = jdi.spectrum_batch([_case(og, df, k) for k, df in enumerate(frames)], opa, calculation="reflected+thermal")
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        _same(g, w)
        assert np.all(np.isfinite(g["albedo"])) and np.all(np.isfinite(g["thermal"]))
    free = _case(og).spectrum(opa, calculation="reflected+thermal")
    assert not np.array_equal(free["albedo"], got[0]["albedo"]) and not np.array_equal(got[0]["albedo"], got[2]["albedo"])
