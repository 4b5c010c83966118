"""The correlated-k factory on the device (csrc/ckfactory.hip through picaso_amd/opacity_factory.py) against the numpy
restatement of the reference's bin loop (test_ck_factory.restate_ck; opacity_factory.py:1927-1955): the selected order
statistics bit for bit, both kernels against each other bit for bit, the coefficients within the rounding of two
logarithms, an analytic case, a directory of rows, and the errors."""
import ctypes

import numpy as np
import pytest

from picaso_amd import _lib
from picaso_amd import opacity_factory as of
from picaso_amd import optics
from picaso_amd.device import DeviceArray
from test_ck_factory import restate_ck, write_directory

pytestmark = pytest.mark.gpu

# 12 000 and 16 384: the last size of the sorting network and the whole LDS array; 16 385: the first length that is selected
# from HBM at the default capacity
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 5000, 12000, 16384, 16385)
G_GAUSS = optics.g_w_2gauss(4, 0.95)[0]
G_EXACT = np.array([0.5, 0.25, 0.75, 0.125, 0.99609375])        # g (n - 1) is an integer for n = 3, 65, 129, 257, ...


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def selection_case():
    """One row; its grid is the point index, so a bin (lo - 0.5, lo + n - 0.5] is the segment [lo, lo + n).  The segments of
    LENGTHS lie one behind the other in a shuffled order with a few unused points between them; two more overlap the
    5 000-point one and each other; one is a single value repeated and one has half its values tied."""
    rng = np.random.default_rng(20240607)
    order = rng.permutation(len(LENGTHS))
    lo, n, at = np.zeros(len(LENGTHS), dtype=np.int64), np.array(LENGTHS, dtype=np.int64), 3
    for b in order:
        lo[b] = at
        at += LENGTHS[b] + 2
    big = lo[LENGTHS.index(5000)]
    lo = np.concatenate((lo, [big + 100, big + 900, at, at + 300]))
    n = np.concatenate((n, [1000, 700, 300, 301]))
    nrow = at + 300 + 301 + 5
    row = 10.0 ** rng.uniform(-300.0, 30.0, nrow)
    special = [0.0, -1.0, -0.0, 5e-324, 1e-310, 1e-200, np.inf, -np.inf, -3e-320, 2.2250738585072014e-308]
    for v in special:
        row[rng.choice(nrow, nrow // 400, replace=False)] = v      # one point in 400 per special value
    row[at:at + 300] = 3.5e-7                                   # a single value repeated
    row[at + 300:at + 601:2] = 1e-200                           # half the values tied (at the clamp value)
    for b in (2, 3, 4):                                         # the shortest segments meet the specials too
        row[lo[b]] = 0.0
        row[lo[b] + 1] = np.inf
    row[lo[1]] = -0.0
    og = np.arange(nrow, dtype=float)
    return dict(row=row, og=og, low=lo - 0.5, high=lo + n - 0.5, lo=lo, n=n)


@pytest.fixture(scope="module")
def runs(selection_case):
    """Every (g set, lds_cap) run of the selection case, made once."""
    c = selection_case
    out = {}
    for name, g in (("gauss", G_GAUSS), ("exact", G_EXACT)):
        for cap in (0, 128):
            out[name, cap] = of.compute_ck(c["row"], c["og"], c["low"], c["high"], g, _lds_cap=cap, _return_stats=True)
    return out


def expected_stats(c, g):
    st = np.full((len(c["lo"]), len(g), 2), 1e-200)
    for b, (lo, n) in enumerate(zip(c["lo"], c["n"])):
        if n < 2:
            continue
        seg = c["row"][lo:lo + n].copy()
        seg[seg <= 0.0] = 1e-200
        seg = np.sort(seg)
        x = np.arange(n) / (n - 1.)
        j = np.searchsorted(x, g, side="right") - 1
        assert np.all((x[j] <= g) & (g < x[j + 1]))
        st[b, :, 0], st[b, :, 1] = seg[j], seg[j + 1]
    return st


@pytest.mark.parametrize("gset", ["gauss", "exact"])
@pytest.mark.parametrize("cap", [0, 128])
def test_selection_is_exact(selection_case, runs, gset, cap):
    c, g = selection_case, (G_GAUSS if gset == "gauss" else G_EXACT)
    lo, n = of.ck_segments(c["og"], c["low"], c["high"])
    assert np.array_equal(lo[n > 0], c["lo"][n > 0]) and np.array_equal(n, c["n"])
    k, stats = runs[gset, cap]
    assert k.shape == (1, len(n), len(g)) and stats.shape == (1, len(n), len(g), 2)
    want = expected_stats(c, g)
    bad = np.argwhere(bits(stats[0]) != bits(want))
    assert bad.size == 0, "first mismatches (bin, gauss, which): %s; segment lengths %s" % (bad[:5], n[bad[:5, 0]])


@pytest.mark.parametrize("gset", ["gauss", "exact"])
def test_lds_and_hbm_paths_agree_bit_for_bit(runs, gset):
    (k0, s0), (k1, s1) = runs[gset, 0], runs[gset, 128]
    assert np.array_equal(bits(s0), bits(s1))
    assert np.array_equal(bits(k0), bits(k1))


@pytest.mark.parametrize("gset", ["gauss", "exact"])
@pytest.mark.parametrize("cap", [0, 128])
def test_coefficients_within_two_logarithms_of_the_restatement(selection_case, runs, gset, cap):
    """|k - restatement| <= 8 * 2^-53 * max(|d[j]|, |d[j+1]|): two logarithms of at most 1 ulp each, carried through an
    interpolation that is numpy's operation for operation.  An infinite order statistic must give numpy's value itself."""
    c, g = selection_case, (G_GAUSS if gset == "gauss" else G_EXACT)
    k, stats = runs[gset, cap]
    k, stats = k[0], stats[0]
    ref = restate_ck(c["row"], c["og"], c["low"], c["high"], g)
    empty = c["n"] < 2
    assert np.all(k[empty] == -200.0) and np.all(ref[empty] == -200.0)
    with np.errstate(all="ignore"):
        d = np.abs(np.log(stats))
        bound = 8.0 * 2.0 ** -53 * np.max(d, axis=2)
        err = np.abs(k - ref)
    finite = np.isfinite(ref) & np.isfinite(bound)
    print("worst |k - ref| / bound over %d finite elements: %.3f" % (finite.sum(), np.max(err[finite] / bound[finite])))
    assert np.array_equal(k[~finite], ref[~finite], equal_nan=True)
    assert finite.sum() > 0.8 * ref.size
    assert np.all(err[finite] <= bound[finite])


def test_constant_bins_give_the_logarithm_of_the_constant():
    """Independent of the restatement: a row that is one constant per bin."""
    rng = np.random.default_rng(5)
    sizes = np.array([2, 3, 64, 129, 777, 2000, 20000])
    const = 10.0 ** rng.uniform(-250.0, 20.0, sizes.size)
    edges = np.concatenate(([0], np.cumsum(sizes)))
    row = np.repeat(const, sizes)
    og = np.arange(row.size, dtype=float)
    for cap in (0, 128):
        k = of.compute_ck(row, og, edges[:-1] - 0.5, edges[1:] - 0.5, G_GAUSS, _lds_cap=cap)[0]
        want = np.log(const)
        assert np.all(np.abs(k - want[:, None]) <= 2.0 * np.spacing(np.abs(want))[:, None])


def element_bound(row, og, low, high, g):
    """``8 * 2^-53 * max(|d[j]|, |d[j+1]|)`` per element from numpy's own sort of the clamped bin; 0 where a bin has fewer
    than two points (those elements are exact)."""
    bound = np.zeros((len(low), len(g)))
    for b, (lo, hi) in enumerate(zip(low, high)):
        seg = row[(og > lo) & (og <= hi)]
        if seg.size < 2:
            continue
        d = np.abs(np.log(np.sort(np.where(seg <= 0.0, 1e-200, seg))))
        j = np.searchsorted(np.arange(seg.size) / (seg.size - 1.), g, side="right") - 1
        bound[b] = 8.0 * 2.0 ** -53 * np.maximum(d[j], d[j + 1])
    return bound


def molecular_case(root, form):
    rng = np.random.default_rng(11)
    pres = [1e-2, 1.0, 100.0] * 2
    temp = [300.0] * 3 + [1200.0] * 3
    numw, file_numbers = 4000, [1, 2, 3, 4, 5, 6]
    rows = [10.0 ** rng.uniform(-40.0, -17.0, numw) * (rng.uniform(size=numw) > 0.02) for _ in file_numbers]
    write_directory(root, "H2O", rows, pres, temp, file_numbers, [numw] * 6, [0.25] * 6, [500.0] * 6, form)
    return rows, np.arange(numw) * 0.25 + 500.0, pres, temp


@pytest.mark.parametrize("form", ["npy", "fortran"])
def test_compute_ck_molecular_on_a_directory_of_rows(tmp_path, form):
    rows, og, pres, temp = molecular_case(str(tmp_path), form)
    new_wno = np.linspace(520.0, 1480.0, 25)
    new_dwno = np.full(25, 40.0)
    new_dwno[3], new_dwno[7] = 90.0, 0.2                        # an overlap and a one-point bin
    table = of.compute_ck_molecular("H2O", str(tmp_path), new_wno=new_wno, new_dwno=new_dwno, verbose=False)
    gi, wi = optics.g_w_2gauss(4, 0.95)
    assert table.shape == (3, 2, 25, 8)
    low, high = 0.5 * (2 * new_wno - new_dwno), 0.5 * (2 * new_wno + new_dwno)
    for idx, row in enumerate(rows):
        ref = restate_ck(row, og, low, high, gi)
        got = table[idx % 3, idx // 3]
        bound = element_bound(row, og, low, high, gi)
        assert np.all(np.isfinite(bound)) and np.all(np.abs(got - ref) <= bound)
        assert np.all(got[ref == -200.0] == -200.0) and np.all(got[7] == -200.0)
    opa = optics.RetrieveCKs(new_wno, wi, pres, temp, [3, 3], kappas={"H2O": table}, gauss_pts=gi)
    assert opa.ngauss == 8 and opa.nwno == 25 and list(opa.molecules) == ["H2O"]


def test_nan_in_a_used_segment_is_an_error_that_names_the_bin_and_outside_is_not():
    rng = np.random.default_rng(2)
    row = 10.0 ** rng.uniform(-30.0, -18.0, 3000)
    og = np.arange(3000, dtype=float)
    low, high = np.array([9.5, 99.5, 999.5, 1999.5]), np.array([59.5, 399.5, 1499.5, 2000.5])
    row[1700] = np.nan                                          # in the gap between bins 2 and 3
    row[5] = np.nan
    clean = of.compute_ck(row, og, low, high, G_GAUSS)
    assert np.all(np.isfinite(clean))
    row[1200] = np.nan
    for cap in (0, 128):                                        # bin 2 has 500 points: sorted in LDS, then selected in HBM
        with pytest.raises(_lib.PicasoHipError, match="NaN in the cross sections of bin 2 "):
            of.compute_ck(row, og, low, high, G_GAUSS, _lds_cap=cap)
    row[2000] = np.nan                                          # the one-point bin 3; the lowest bin is named
    with pytest.raises(_lib.PicasoHipError, match="bin 2 "):
        of.compute_ck(row, og, low, high, G_GAUSS)
    row[1200] = 1e-20
    with pytest.raises(_lib.PicasoHipError, match="bin 3 "):
        of.compute_ck(row, og, low, high, G_GAUSS)
    row[2000] = 1e-20
    assert np.array_equal(of.compute_ck(row, og, low, high, G_GAUSS), clean)      # the context is fine afterwards


def test_bad_segments_and_arguments_fail_cleanly_in_the_entry_point():
    ctx, lib = _lib.context(), _lib.load()
    d_row = DeviceArray.from_host(np.ones(100), ctx)
    d_k = DeviceArray((2, 8), ctx)
    ll = ctypes.POINTER(ctypes.c_longlong)

    def call(lo, n, g=G_GAUSS, n_lbl=100, cap=0, row=d_row.addr):
        lo, n, g = np.array(lo, dtype=np.int64), np.array(n, dtype=np.int64), np.array(g, dtype=float)
        return lib.picaso_ck_from_xsec_dev(ctx, ctypes.c_long(n_lbl), ctypes.c_void_p(row), ctypes.c_int(len(lo)),
                                           lo.ctypes.data_as(ll), n.ctypes.data_as(ll), ctypes.c_int(len(g)), _lib.ptr(g),
                                           ctypes.c_long(cap), ctypes.c_void_p(d_k.addr), None)

    for kwargs, msg in ((dict(lo=[0, 60], n=[10, 41]), "bin 1"), (dict(lo=[0, 5], n=[-1, 5]), "negative count"),
                        (dict(lo=[-1, 5], n=[2, 5]), "bin 0"), (dict(lo=[0, 101], n=[2, 0]), "bin 1"),
                        (dict(lo=[0, 5], n=[2, 5], g=[0.5, 1.0]), r"outside \(0, 1\)"),
                        (dict(lo=[0, 5], n=[2, 5], g=[0.0]), r"outside \(0, 1\)"),
                        (dict(lo=[0, 5], n=[2, 5], g=[]), "ngauss"), (dict(lo=[0, 5], n=[2, 5], g=[0.5] * 33), "ngauss"),
                        (dict(lo=[0, 5], n=[2, 5], cap=16385), "lds_cap"), (dict(lo=[0, 5], n=[2, 5], cap=-1), "lds_cap"),
                        (dict(lo=[0] * 262145, n=[0] * 262145), "at most 262144"),
                        (dict(lo=[0, 5], n=[2, 5], n_lbl=0), "n_lbl"), (dict(lo=[0, 5], n=[2, 5], row=None), "NULL")):
        assert call(**kwargs) != 0
        with pytest.raises(_lib.PicasoHipError, match=msg):
            _lib.check(1, ctx)
    assert call(lo=[0, 60], n=[10, 40]) == 0                    # the last point of the row may be used
    assert np.all(d_k.to_host() == 0.0)                         # ln(1) everywhere
