"""``picaso_amd.chemistry`` on the host: the readers, the choice of the grid file, ``ChemTable``'s refusals and the numpy form
``interp_numpy`` against the reference's own ``chem_interp`` (tests/golden/chemistry.npz, tests/golden/chemistry/:
tests/golden/make_chemistry.py).

Tolerance against the reference: ``interp_numpy`` is the body of ``inputs.chem_interp``, which tests/test_climate_driver_host.py
holds to 1e-12 relative against scipy; the reference forms the same bilinear expression with its four terms grouped the same
way but its index arithmetic in another order, so the same 1e-12 is asked of the abundance here.  (An abundance is
``10**x``; a difference of a few ulp in ``x ~ -50`` is ``50 * 2.3 * 2^-52 ~ 3e-14`` relative.)
"""
import os
import shutil

import numpy as np
import pytest

from helpers import GOLDEN

CHEM_DIR = os.path.join(GOLDEN, "chemistry")
DIR_2121 = os.path.join(CHEM_DIR, "visscher_grid_2121")
DIR_1060 = os.path.join(CHEM_DIR, "visscher_grid_1060")
FILE_2121 = "sonora_2121grid_feh0.0_co0.55.txt"
FILE_1060 = "2015_06_1060grid_feh_00_co_10.txt"
FILE_LOW = "visscher_abunds_m+0.0_co1.0"
RTOL_REFERENCE = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "chemistry.npz"))


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(CHEM_DIR, "expected.npz"))


def table_of(gold, tag):
    """The columns dictionary of a stored table, in file order."""
    return {str(k): gold["%s/%s" % (tag, k)] for k in gold[tag + "/columns"]}


def ragged_1060(gold):
    """The 1060 table with the top pressures of some temperatures dropped: ``nc_p`` varies, every ``nc_p >= 3``."""
    tab = table_of(gold, "t1060")
    temps = np.unique(tab["temperature"])
    keep = np.ones(len(tab["temperature"]), dtype=bool)
    for it, t in enumerate(temps):
        rows = np.flatnonzero(tab["temperature"] == t)
        drop = (0, 3, 7, len(rows) - 3, 1)[it % 5]                      # up to all but three
        if drop:
            keep[rows[len(rows) - drop:]] = False
    return {k: v[keep] for k, v in tab.items()}


def species_of(expected, case, grid):
    pre = "%s/%s/" % (case, grid)
    return [k[len(pre):] for k in expected.files if k.startswith(pre)]


# ------------------------------------------------------------------------------------------------------ readers
def _same_columns(got, gold, tag):
    assert list(got.keys()) == [str(k) for k in gold[tag + "/columns"]]
    for k, v in got.items():
        assert v.dtype == np.float64 and np.array_equal(v, gold["%s/%s" % (tag, k)]), k


def test_readers_give_the_reference_columns_bit_for_bit(gold):
    from picaso_amd import chemistry as ch
    _same_columns(ch.read_visscher_2121(os.path.join(DIR_2121, FILE_2121)), gold, "cut2121")
    _same_columns(ch.read_visscher_1060(os.path.join(DIR_1060, FILE_1060)), gold, "cut1060")
    low = ch.read_channon_grid_low(os.path.join(CHEM_DIR, FILE_LOW))
    _same_columns(low, gold, "cutlow")
    assert "pressure" in low and "temperature" in low and "" not in low          # the index column is gone
    # the cut-down file holds the first rows of the full one
    full = table_of(gold, "t2121")
    cut = ch.read_visscher_2121(os.path.join(DIR_2121, FILE_2121))
    n = len(cut["pressure"])
    assert n == 42 and len(np.unique(cut["temperature"])) == 2
    assert all(np.array_equal(cut[k], full[k][:n]) for k in full)
    assert cut["pressure"][0] == 10 ** -6.0 or np.isclose(cut["pressure"].min(), full["pressure"].min())


def test_a_reader_refuses_a_file_whose_rows_do_not_match_its_header(tmp_path):
    from picaso_amd import chemistry as ch
    path = tmp_path / "bad.txt"
    path.write_text("T(K) P(bar) H2 He\n100.0 -6.0 0.8\n100.0 -5.0 0.8\n")
    with pytest.raises(ValueError, match="header"):
        ch.read_visscher_2121(str(path))


# ------------------------------------------------------------------------------------------------------ file selection
def test_visscher_2121_chooses_the_file_the_reference_chooses(gold):
    from picaso_amd import chemistry as ch
    for (co, mh), want in zip(gold["sel2121/targets"], gold["sel2121/chosen"]):
        got = ch.select_visscher_2121(float(co), float(mh), directory=DIR_2121)
        assert os.path.basename(got) == str(want), (co, mh)
    # the last target is the tie that sorted order decides
    co, mh = gold["sel2121/targets"][-1]
    names = sorted(os.listdir(DIR_2121))
    tied = [n for n in names if n in ("sonora_2121grid_feh0.0_co0.55.txt", "sonora_2121grid_feh0.5_co0.55.txt")]
    assert len(tied) == 2 and os.path.basename(ch.select_visscher_2121(float(co), float(mh), DIR_2121)) == tied[0]
    tab = ch.visscher_2121(0.6, 0.1, directory=DIR_2121)
    assert np.array_equal(tab["H2O"], gold["cut2121/H2O"])


def test_visscher_2121_default_directory_and_errors(tmp_path, monkeypatch):
    from picaso_amd import chemistry as ch
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="visscher_grid_2121"):
        ch.visscher_2121(0.55, 0.0)
    shutil.copytree(DIR_2121, str(tmp_path / "chemistry" / "visscher_grid_2121"))
    assert os.path.basename(ch.select_visscher_2121(0.55, 0.0)) == FILE_2121
    assert "H2O" in ch.visscher_2121(0.55, 0.0)
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("nothing here\n")
    with pytest.raises(Exception, match="No files matching"):
        ch.visscher_2121(0.55, 0.0, directory=str(empty))


def test_visscher_1060_builds_the_reference_file_name(gold):
    from picaso_amd import chemistry as ch
    for (co, mh), want in zip(gold["sel1060/targets"], gold["sel1060/chosen"]):
        want = str(want)
        if want.startswith("raises: "):
            with pytest.raises(Exception) as err:
                ch.select_visscher_1060(float(co), float(mh), directory=DIR_1060)
            assert str(err.value) == want[len("raises: "):]
        else:
            assert os.path.basename(ch.select_visscher_1060(float(co), float(mh), directory=DIR_1060)) == want, (co, mh)
    tab = ch.visscher_1060(1.0, 0.0, directory=DIR_1060)
    assert np.array_equal(tab["CH4"], gold["cut1060/CH4"])


# ------------------------------------------------------------------------------------------------------ ChemTable refusals
def _small_table(temps, nc_p, press=None):
    press = np.logspace(-3, 1, 5) if press is None else press
    rows_t = np.concatenate([[t] * n for t, n in zip(temps, nc_p)])
    rows_p = np.concatenate([press[:n] for n in nc_p])
    return {"pressure": rows_p, "temperature": rows_t, "H2": np.full(len(rows_t), 0.8), "He": np.full(len(rows_t), 0.2)}


@pytest.mark.parametrize("table,reason", [
    (_small_table([500.0], [5]), "temperature"),
    (_small_table([500.0, 900.0], [5, 5], press=np.array([-1.0, 0.0, 1.0, 0.0, -1.0])), "positive pressure"),
    (_small_table([500.0, 900.0, 1300.0], [5, 2, 5]), "needs three"),
    (dict(_small_table([500.0, 900.0], [5, 5]), pressure=np.tile(np.logspace(-3, 1, 5)[[0, 0, 1, 1, 2]], 2)), "only 3 positive"),
    (dict(_small_table([500.0, 900.0], [5, 5]), H2=np.full(9, 0.8), He=np.full(9, 0.2)), "add up to"),
])
def test_chem_table_refuses_what_its_clamps_could_not_hold(table, reason):
    """The checks run before anything touches the device, so they need none."""
    from picaso_amd import chemistry as ch
    with pytest.raises(ValueError, match=reason):
        ch.ChemTable(table, ctx=object())


def test_chem_table_refuses_a_table_without_its_axes():
    from picaso_amd import chemistry as ch
    with pytest.raises(ValueError, match="pressure"):
        ch.ChemTable({"temperature": np.ones(3), "H2": np.ones(3)}, ctx=object())
    with pytest.raises(ValueError, match="no species"):
        ch.ChemTable({"temperature": np.ones(3), "pressure": np.ones(3)}, ctx=object())


# ------------------------------------------------------------------------------------------------------ the numpy form
@pytest.mark.parametrize("case", ["hj", "scatter"])
@pytest.mark.parametrize("grid", ["2121", "1060", "low"])
def test_interp_numpy_against_the_reference(gold, expected, case, grid):
    from picaso_amd import chemistry as ch
    tab = table_of(gold, "t" + grid)
    t, p = expected[case + "/temperature"], expected[case + "/pressure"]
    species, got = ch.interp_numpy(t, p, tab)
    assert species == species_of(expected, case, grid) == [k for k in tab if k not in ("temperature", "pressure")]
    assert got.shape == (len(t), len(species))
    worst = 0.0
    for i, sp in enumerate(species):
        want = expected["%s/%s/%s" % (case, grid, sp)]
        assert np.array_equal(np.isfinite(want), np.isfinite(got[:, i])) and np.array_equal(want == 0, got[:, i] == 0), sp
        ok = np.isfinite(want) & (want != 0)
        worst = max(worst, float(np.max(np.abs(got[ok, i] - want[ok]) / np.abs(want[ok]))))
    print("%s on %s: worst relative distance from the reference %.2e" % (case, grid, worst))
    assert worst <= RTOL_REFERENCE


def test_interp_numpy_exponent_is_the_abundance_exponent(gold, expected):
    from picaso_amd import chemistry as ch
    tab = table_of(gold, "t2121")
    t, p = expected["scatter/temperature"], expected["scatter/pressure"]
    _, x = ch.interp_numpy(t, p, tab, log10=True)
    _, a = ch.interp_numpy(t, p, tab)
    assert np.array_equal(10 ** x, a)


def test_interp_numpy_on_a_ragged_table_keeps_every_row_inside(gold, expected):
    from picaso_amd import chemistry as ch
    tab = ragged_1060(gold)
    species, _, _, p_log_grid, nc_p, start = ch.table_grids(tab)
    assert nc_p.min() == 3 and len(np.unique(nc_p)) > 3 and start[-1] == len(tab["pressure"]) and nc_p.max() <= len(p_log_grid)
    t, p = expected["scatter/temperature"][:257], expected["scatter/pressure"][:257]
    _, got = ch.interp_numpy(t, p, tab)
    assert got.shape == (257, len(species)) and np.all(np.isfinite(got))


# ------------------------------------------------------------------------------------------------------ inputs.chem_interp
def _chem_interp_before_the_move(prof, chem_grid):
    """``inputs.chem_interp`` as it stood before its body moved to ``chemistry.interp_numpy``, kept here word for word as the
    record of 'unchanged'."""
    plevel, tlevel = np.asarray(prof["pressure"], dtype=float), np.asarray(prof["temperature"], dtype=float)
    t_inv, p_log = 1 / tlevel, np.log10(plevel)
    tab_t, tab_p = np.asarray(chem_grid["temperature"], dtype=float), np.asarray(chem_grid["pressure"], dtype=float)
    species = [k for k in chem_grid.keys() if k not in ("pressure", "temperature")]
    with np.errstate(divide="ignore"):
        log_abunds = np.log10(np.stack([np.asarray(chem_grid[k], dtype=float) for k in species], axis=1))
    nc_p = np.unique(tab_t, return_counts=True)[1]
    _, first = np.unique(tab_t, return_index=True)
    temps = tab_t[np.sort(first)]
    p_grid = np.unique(tab_p)
    p_log_grid = np.log10(p_grid[p_grid > 0])
    t_inv_grid = 1 / temps
    nt = len(t_inv_grid)

    def last_where(mask):
        idx = mask.shape[1] - 1 - np.argmax(mask[:, ::-1], axis=1)
        return np.where(mask.any(axis=1), idx, 0)
    t_low = last_where(t_inv_grid[None, :] > t_inv[:, None])
    t_low[t_low == nt - 1] = nt - 2
    t_hi = t_low + 1
    p_low = np.minimum(last_where(p_log_grid[None, :] <= p_log[:, None]), nc_p[t_hi] - 3)
    p_hi = p_low + 1
    start = np.concatenate(([0], np.cumsum(nc_p)))
    t_i = ((t_inv - t_inv_grid[t_low]) / (t_inv_grid[t_hi] - t_inv_grid[t_low]))[:, None]
    p_i = ((p_log - p_log_grid[p_low]) / (p_log_grid[p_hi] - p_log_grid[p_low]))[:, None]
    abunds = 10 ** (((1 - t_i) * (1 - p_i) * log_abunds[start[t_low] + p_low, :])
                    + (t_i * (1 - p_i) * log_abunds[start[t_hi] + p_low, :])
                    + (t_i * p_i * log_abunds[start[t_hi] + p_hi, :])
                    + ((1 - t_i) * p_i * log_abunds[start[t_low] + p_hi, :]))
    return {k: abunds[:, i] for i, k in enumerate(species)}


def test_inputs_chem_interp_is_unchanged_by_the_move(gold, expected):
    from picaso_amd import justdoit as jdi
    t, p = expected["hj/temperature"], expected["hj/pressure"]
    for tag in ("t2121", "t1060"):
        tab = table_of(gold, tag)
        b = jdi.inputs(calculation="browndwarf")
        b.add_pt(t, p)
        prof = b.inputs["atmosphere"]["profile"]
        want = _chem_interp_before_the_move(prof, tab)
        b.chem_interp(tab)
        assert list(prof.keys()) == ["temperature", "pressure"] + list(want)
        assert all(np.array_equal(prof[k], v) for k, v in want.items())


def test_the_one_d_route_and_channon_grid_low(gold, expected, tmp_path, monkeypatch):
    """``case.chem_interp(chemistry.visscher_2121(...))`` on the cut-down directory, and ``channon_grid_low`` from a file and
    from ``$picaso_refdata``: each equals ``interp_numpy`` on the table its reader returns."""
    from picaso_amd import chemistry as ch
    from picaso_amd import justdoit as jdi
    t, p = np.array([80.0, 95.0, 120.0]), np.array([1e-5, 3e-3, 2.0])
    b = jdi.inputs(calculation="browndwarf")
    b.add_pt(t, p)
    b.chem_interp(ch.visscher_2121(0.55, 0.0, directory=DIR_2121))
    species, want = ch.interp_numpy(t, p, table_of(gold, "cut2121"))
    assert all(np.array_equal(b.inputs["atmosphere"]["profile"][k], want[:, i]) for i, k in enumerate(species))
    low = table_of(gold, "cutlow")
    species, want = ch.interp_numpy(t, p, low)
    b.add_pt(t, p)
    b.channon_grid_low(os.path.join(CHEM_DIR, FILE_LOW))
    prof = b.inputs["atmosphere"]["profile"]
    assert list(prof.keys()) == ["temperature", "pressure"] + species
    assert all(np.array_equal(prof[k], want[:, i]) for i, k in enumerate(species))
    shutil.copytree(CHEM_DIR, str(tmp_path / "chemistry"))
    monkeypatch.setenv("picaso_refdata", str(tmp_path))
    b.add_pt(t, p)
    b.channon_grid_low()
    assert all(np.array_equal(b.inputs["atmosphere"]["profile"][k], want[:, i]) for i, k in enumerate(species))


# ------------------------------------------------------------------------------------------------------ 3-D, without a device
def test_chemeq_3d_and_premix_3d_say_what_is_missing():
    from picaso_amd import justdoit as jdi
    c = jdi.inputs()
    with pytest.raises(Exception, match="atmosphere_3d"):
        c.chemeq_3d()
    with pytest.raises(Exception, match="atmosphere_3d"):
        c.premix_3d(type("Opa", (), {"full_abunds": {"pressure": np.ones(3)}})())
    with pytest.raises(Exception, match="full_abunds"):
        c.premix_3d(object())
    with pytest.warns(UserWarning, match="cto_absolute"), pytest.raises(Exception, match="atmosphere_3d"):
        c.chemeq_3d(c_o=1.0)


def test_chem_interp_batch_checks_its_arguments_before_the_device(gold):
    from picaso_amd import chemistry as ch
    with pytest.raises(ValueError, match="shape"):
        ch.chem_interp_batch(np.ones(3), np.ones(4), table_of(gold, "cut2121"))
    with pytest.raises(ValueError, match="out must be"):
        ch.chem_interp_batch(np.ones(3), np.ones(3), table_of(gold, "cut2121"), out="pinned")
