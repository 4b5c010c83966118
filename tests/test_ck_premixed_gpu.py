"""Premixed correlated-k tables on the device (csrc/xsecsum.hip and csrc/ckfactory.hip through
picaso_amd/opacity_factory.py): the abundance-weighted sum against numpy's ``s = 0; s += w * d`` bit for bit, with and
without ``np.interp`` onto the grid of the sum, the entry point's refusals, and ``compute_ck_premixed`` on a directory of
gases against the numpy restatement of the reference's bin loop applied to the numpy sum."""
import numpy as np
import pytest

from helpers import h5py_module
from picaso_amd import _lib
from picaso_amd import opacity_factory as of
from picaso_amd import optics
from picaso_amd.device import DeviceArray
from test_ck_factory import restate_ck, write_directory
from test_ck_factory_gpu import bits, element_bound

pytestmark = pytest.mark.gpu

WEIGHTS = (0.0, 1e-50, 0.3, 1.0)
GASES = ["H2O", "CH4", "CO"]


def numpy_sum(rows, weights):
    """The reference's loop (opacity_factory.py:1617, 1713)."""
    s = 0
    with np.errstate(all="ignore"):
        for w, d in zip(weights, rows):
            s += np.float64(w) * d
    return s


def xsec_rows(rng, n, m=3):
    """``m`` rows of ``10**uniform(-40, -17)`` with exact zeros, a -0.0, a 1e-100 and a 1e-300 (times 1e-50 it vanishes),
    and a 1e-270 (times 1e-50 it is subnormal)."""
    rows = [10.0 ** rng.uniform(-40.0, -17.0, n) for _ in range(m)]
    special = (0.0, -0.0, 1e-100, 1e-300, 1e-270, 4e-308)
    for r, row in enumerate(rows):
        row[rng.uniform(size=n) < 0.05] = 0.0
        if n > 2 * len(special):
            row[1 + r:1 + r + len(special)] = special
            row[n - 1] = special[(r + 3) % len(special)]       # the odd tail element at odd n
    rows[0][0] = -0.0                               # the first product of the sum: 0.0 + -0.0 = +0.0
    return rows


WEIGHT_SETS = ((0.3, 1e-50, 1.0), (1e-50, 0.0, 0.3), (0.0, 1.0, 1e-50), (1.0, 0.3, 0.0), (1e-50, 1e-50, 1e-50))


@pytest.mark.parametrize("n_out", [1, 63, 64, 65, 257, 4097])
def test_sum_is_numpys_bit_for_bit(n_out):
    rng = np.random.default_rng(100 + n_out)
    rows = xsec_rows(rng, n_out)
    assert set(w for ws in WEIGHT_SETS for w in ws) == set(WEIGHTS)
    tiny = 0
    for weights in WEIGHT_SETS:
        want = numpy_sum(rows, weights)
        got = of.weighted_sum(rows, weights)
        assert got.shape == (n_out,) and np.array_equal(bits(got), bits(want)), weights
        tiny += int(np.sum((want != 0.0) & (np.abs(want) < 2.2250738585072014e-308)))
    assert n_out == 1 or tiny > 0                                           # subnormal products and sums were met
    assert bits(of.weighted_sum([rows[0]], [1.0]))[0] == 0                  # 0.0 + -0.0: +0.0
    d = of.weighted_sum(rows, WEIGHT_SETS[0], out="device")                 # the same sum left on the device
    assert isinstance(d, DeviceArray) and np.array_equal(bits(d.to_host()), bits(numpy_sum(rows, WEIGHT_SETS[0])))
    d.free()


def test_unaligned_buffers_take_the_scalar_kernel_with_the_same_bits():
    rng = np.random.default_rng(7)
    n = 1001
    rows = xsec_rows(rng, n, 2)
    ctx, lib = _lib.context(), _lib.load()
    d_src = [DeviceArray.from_host(np.concatenate(([9.0], r)), ctx) for r in rows]
    d_acc = DeviceArray.from_host(np.full(n + 2, 7.0), ctx)
    for m, w in enumerate((0.3, 1e-50)):
        _lib.check(lib.picaso_xsec_axpy_dev(ctx, n, d_acc.addr + 8, int(m == 0), w, d_src[m].addr + 8, n, None, None, 0.0,
                                            0.0), ctx)
    got = d_acc.to_host()
    assert got[0] == 7.0 and got[-1] == 7.0                                 # nothing outside [1, n + 1) was written
    assert np.array_equal(bits(got[1:-1]), bits(numpy_sum(rows, (0.3, 1e-50))))


@pytest.fixture(scope="module")
def interp_case():
    """An ``out_grid`` of 4 097 points and source grids that are coarser, finer, shifted, inside it (both clamps), share
    every fourth knot with it exactly, hold two equal neighbouring values (zero slope), and are not uniform (the guessed
    bracket is wrong by many knots: the binary search takes over)."""
    rng = np.random.default_rng(42)
    out_grid = of.uniform_grid(4097, 0.25, 500.0)                           # multiples of 0.25: exact
    grids = {
        "coarser": of.uniform_grid(1500, 0.7, 499.0),
        "finer": of.uniform_grid(9000, 0.117, 498.3),
        "shifted": of.uniform_grid(4097, 0.25, 500.1),
        "middle": of.uniform_grid(2000, 0.2, 800.0),                        # [800, 1199.8] of [500, 1524]
        "every_fourth_knot": of.uniform_grid(1025, 1.0, 500.0),
        "zero_slope": of.uniform_grid(3000, 0.35, 499.9),
        "not_uniform": np.sort(np.concatenate(([499.0, 1600.0], 500.0 + 1024.0 * rng.uniform(size=2500) ** 3))),
        "same": out_grid.copy(),                                            # array_equal: not interpolated
    }
    rows = {k: 10.0 ** rng.uniform(-40.0, -17.0, g.size) * (rng.uniform(size=g.size) > 0.03) for k, g in grids.items()}
    rows["zero_slope"][100:104] = 3.5e-21
    rows["zero_slope"][200:202] = 0.0
    assert np.array_equal(grids["every_fourth_knot"], out_grid[::4])
    return out_grid, grids, rows


def test_interpolated_sum_is_numpys_bit_for_bit(interp_case):
    out_grid, grids, rows = interp_case
    names = list(grids)
    weights = [0.3, 1.0, 1e-50, 0.7, 1.0, 2.0, 0.25, 0.5]
    on_grid = [np.interp(out_grid, grids[k], rows[k]) if of.are_arrays_different(out_grid, grids[k]) else rows[k]
               for k in names]
    hits = np.isin(out_grid, grids["every_fourth_knot"]).sum()
    assert hits == 1025 and out_grid[0] < grids["middle"][0] and out_grid[-1] > grids["middle"][-1]
    want = numpy_sum(on_grid, weights)
    got = of.weighted_sum([rows[k] for k in names], weights, grids=[grids[k] for k in names], out_grid=out_grid)
    assert np.array_equal(bits(got), bits(want))
    for k in names:                                                         # one grid at a time: a failure names it
        got = of.weighted_sum([rows[k]], [1.0], grids=[grids[k]], out_grid=out_grid)
        bad = np.nonzero(bits(got) != bits(numpy_sum([on_grid[names.index(k)]], [1.0])))[0]
        assert bad.size == 0, (k, bad[:5], out_grid[bad[:5]])
    # a row as long as its grid says, or an error that names it
    with pytest.raises(Exception, match="row 0 has 1500 points, its wavenumber grid 9000"):
        of.weighted_sum([rows["coarser"]], [1.0], grids=[grids["finer"]], out_grid=out_grid)
    with pytest.raises(Exception, match="ascending"):
        of.weighted_sum([rows["coarser"]], [1.0], grids=[grids["coarser"][::-1]], out_grid=out_grid)


def test_bad_arguments_fail_cleanly_in_the_entry_point_and_the_context_lives_on():
    ctx, lib = _lib.context(), _lib.load()
    src = np.arange(1.0, 101.0)
    d_src, d_acc = DeviceArray.from_host(src, ctx), DeviceArray.from_host(np.full(100, 5.0), ctx)
    d_grid = DeviceArray.from_host(np.arange(100.0), ctx)

    def call(n_out=100, first=1, weight=1.0, n_src=100, src_grid=None, out_grid=None, acc=d_acc.addr, src=d_src.addr):
        return lib.picaso_xsec_axpy_dev(ctx, n_out, acc, first, weight, src, n_src, src_grid, out_grid, 0.0, 0.0)

    for kwargs, msg in ((dict(weight=float("nan")), "weight is NaN"), (dict(n_src=99), "99 points, the sum 100"),
                        (dict(n_out=99), "100 points, the sum 99"), (dict(n_out=0, n_src=0), "n_out must be positive"),
                        (dict(n_src=1, src_grid=d_grid.addr, out_grid=d_grid.addr), "at least 2 knots"),
                        (dict(n_out=2 ** 31, n_src=2 ** 31), "at most 2147483647"),
                        (dict(src_grid=d_grid.addr), "go together"), (dict(acc=None), "NULL"), (dict(src=None), "NULL")):
        assert call(**kwargs) != 0
        with pytest.raises(_lib.PicasoHipError, match=msg):
            _lib.check(1, ctx)
    assert np.all(d_acc.to_host() == 5.0)                                   # nothing was launched
    with pytest.raises(Exception, match="row 1 has 3 points, the sum 4"):
        of.weighted_sum([np.ones(4), np.ones(3)], [1.0, 1.0])
    assert call(first=0, weight=2.0) == 0
    assert np.array_equal(d_acc.to_host(), 5.0 + 2.0 * src)
    assert np.array_equal(of.weighted_sum([src, src], [1.0, 0.5]), src + 0.5 * src)


def mixture_case(root, forms):
    """3 gases x 6 P-T points of 4 000 points, and the abundances (exactly 6 rows: taken as they stand)."""
    rng = np.random.default_rng(11)
    pres = [1e-2, 1.0, 100.0] * 2
    temp = [300.0] * 3 + [1200.0] * 3
    numw, file_numbers = 4000, [1, 2, 3, 4, 5, 6]
    rows = {}
    for gas, form in zip(GASES, forms):
        rows[gas] = [10.0 ** rng.uniform(-40.0, -17.0, numw) * (rng.uniform(size=numw) > 0.3) for _ in file_numbers]
        write_directory(root, gas, rows[gas], pres, temp, file_numbers, [numw] * 6, [0.25] * 6, [500.0] * 6, form)
    chem = {"temperature": np.array(temp), "pressure": np.array(pres), "H2O": rng.uniform(1e-4, 1e-3, 6),
            "CH4": 10.0 ** rng.uniform(-30.0, -4.0, 6), "CO": rng.uniform(1e-5, 1e-4, 6)}
    sums = [numpy_sum([rows[g][i] for g in GASES], [chem[g][i] for g in GASES]) for i in range(6)]
    new_wno = np.linspace(520.0, 1480.0, 25)
    new_dwno = np.full(25, 40.0)
    new_dwno[3], new_dwno[7], new_dwno[11] = 90.0, 0.2, 0.01        # an overlap, a one-point bin and an empty one
    new_wno[11] += 0.1                                              # ... between two points of the rows' grid
    return rows, chem, sums, np.arange(numw) * 0.25 + 500.0, pres, temp, new_wno, new_dwno


@pytest.mark.parametrize("forms", [("npy",) * 3, ("fortran",) * 3], ids=["npy", "fortran"])
def test_compute_ck_premixed_on_a_directory_of_gases(tmp_path, forms):
    rows, chem, sums, og, pres, temp, new_wno, new_dwno = mixture_case(str(tmp_path), forms)
    table = of.compute_ck_premixed(GASES, str(tmp_path), chem, new_wno=new_wno, new_dwno=new_dwno, verbose=False)
    gi = optics.g_w_2gauss(4, 0.95)[0]
    assert table.shape == (3, 2, 25, 8)
    low, high = 0.5 * (2 * new_wno - new_dwno), 0.5 * (2 * new_wno + new_dwno)
    n_in = [int(np.sum((og > a) & (og <= b))) for a, b in zip(low, high)]
    assert n_in[7] == 1 and n_in[11] == 0
    for idx, s in enumerate(sums):
        ref = restate_ck(s, og, low, high, gi)
        got = table[idx % 3, idx // 3]
        bound = element_bound(s, og, low, high, gi)
        err = np.abs(got - ref)
        print("point %d: worst |k - ref| / bound %.3f" % (idx, np.max(err[bound > 0] / bound[bound > 0])))
        assert np.all(np.isfinite(bound)) and np.all(err <= bound)
        assert np.all(got[ref == -200.0] == -200.0) and np.all(got[7] == -200.0) and np.all(got[11] == -200.0)
    hbm = of.compute_ck_premixed(GASES, str(tmp_path), chem, new_wno=new_wno, new_dwno=new_dwno, verbose=False, _lds_cap=128)
    assert max(n_in) > 128 and np.array_equal(bits(hbm), bits(table))


def test_one_gas_with_weight_one_is_compute_ck_molecular_bit_for_bit(tmp_path):
    rows, chem, sums, og, pres, temp, new_wno, new_dwno = mixture_case(str(tmp_path), ("npy", "fortran", "npy"))
    chem = dict(chem, CH4=np.ones(6))
    one = of.compute_ck_premixed(["CH4"], str(tmp_path), chem, new_wno=new_wno, new_dwno=new_dwno, verbose=False)
    ref = of.compute_ck_molecular("CH4", str(tmp_path), new_wno=new_wno, new_dwno=new_dwno, verbose=False)
    assert np.array_equal(bits(one), bits(ref))


def test_two_constant_gases_give_the_logarithm_of_the_weighted_constants(tmp_path):
    """Independent of the restatement: two gases that are one constant per bin."""
    rng = np.random.default_rng(5)
    sizes = np.array([2, 3, 64, 129, 777, 2000, 20000])
    edges = np.concatenate(([0], np.cumsum(sizes)))
    ca, cb = 10.0 ** rng.uniform(-30.0, -17.0, sizes.size), 10.0 ** rng.uniform(-30.0, -17.0, sizes.size)
    wa, wb = 3.1e-4, 0.86
    numw = int(edges[-1])
    for gas, c in (("H2O", ca), ("H2", cb)):
        write_directory(str(tmp_path), gas, [np.repeat(c, sizes)], [1.0], [500.0], [1], [numw], [1.0], [0.0])
    chem = {"temperature": np.array([500.0]), "pressure": np.array([1.0]), "H2O": np.array([wa]), "H2": np.array([wb])}
    new_wno, new_dwno = 0.5 * (edges[:-1] + edges[1:]) - 0.5, sizes.astype(float)       # bins (e0 - 0.5, e1 - 0.5]
    want = np.log(wa * ca + wb * cb)
    for cap in (0, 128):
        k = of.compute_ck_premixed(["H2O", "H2"], str(tmp_path), chem, new_wno=new_wno, new_dwno=new_dwno, verbose=False,
                                   _lds_cap=cap)
        assert k.shape == (1, 1, sizes.size, 8)
        assert np.all(np.abs(k[0, 0] - want[:, None]) <= 2.0 * np.spacing(np.abs(want))[:, None])


def test_premixed_file_round_trip_into_retrieve_cks(tmp_path, monkeypatch):
    import sys
    mod, stub = h5py_module()
    if stub:
        monkeypatch.setitem(sys.modules, "h5py", mod)
    root = tmp_path / "xsec"
    rows, chem, sums, og, pres, temp, new_wno, new_dwno = mixture_case(str(root), ("npy", "npy", "fortran"))
    table = of.compute_ck_premixed(GASES, str(root), chem, new_wno=new_wno, new_dwno=new_dwno, verbose=False)
    path = str(tmp_path / "premixed.hdf5")
    assert of.compute_ck_premixed(GASES, str(root), chem, new_wno=new_wno, new_dwno=new_dwno, climate_filename=path,
                                  verbose=False) is None
    t = optics.read_ck_tables(path)
    assert np.array_equal(bits(t["kappa"]), bits(table)) and t["molecules"] == GASES
    assert t["abunds_map"] == list(chem) and np.array_equal(t["abunds"], np.column_stack([chem[c] for c in chem]))
    with mod.File(path, "r") as f:
        assert np.array_equal(f["nc_p"][:], [3.0, 3.0])                    # as compute_ck_molecular's
    assert np.array_equal(t["nc_p"], [3, 3])
    opa = optics.RetrieveCKs(t["wno"], t["gauss_wts"], t["pressures"], t["temps"], t["nc_p"], ln_kappa=t["kappa"],
                             gauss_pts=t["gauss_pts"])
    assert opa.ngauss == 8 and opa.nwno == 25
