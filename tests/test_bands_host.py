"""``picaso_amd.retrieval`` on the host against tests/golden/bands.npz -- scipy's ``mquantiles`` and the reference's own
``get_evaluations`` / ``get_chisq_max`` on tests/bands_cases.py's inputs (tests/golden/make_bands.py).  The device call
(``retrieval._reduce``) is replaced by bands_cases' ``np.sort`` restatement, which the GPU tests hold the kernel to."""
import os

import numpy as np
import pytest

import bands_cases as bc
from helpers import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "bands.npz"))


@pytest.fixture
def on_host(monkeypatch):
    """``retrieval`` with its device call replaced by the numpy restatement; records the shapes it was called with."""
    from picaso_amd import retrieval
    calls = []

    def reduce_numpy(ys, k, gamma):
        calls.append(np.shape(ys))
        return bc.lines_numpy(ys, k, gamma)
    monkeypatch.setattr(retrieval, "_reduce", reduce_numpy)
    monkeypatch.setattr(retrieval, "calls", calls, raising=False)
    return retrieval


def test_sigma_quantiles_are_the_references_levels():
    from picaso_amd import retrieval
    assert tuple(retrieval.SIGMA_QUANTILES.keys()) == bc.KEYS
    assert list(retrieval.SIGMA_QUANTILES.values()) == bc.LEVELS


@pytest.mark.parametrize("S", bc.FIXTURE_DRAWS)
def test_quantile_table_reproduces_mquantiles(gold, S):
    from picaso_amd import retrieval
    y = bc.fixture_matrix(S)
    assert np.array_equal(y.ravel()[::5], gold["M%d/in_probe" % S], equal_nan=True)
    k, gamma = retrieval.quantile_table(S, bc.LEVELS)
    assert k.dtype == np.int32 and gamma.dtype == np.float64 and k.shape == gamma.shape == (7,)
    want = gold["M%d/bands" % S]
    assert np.isnan(want[:, 5]).any() and not np.isnan(np.delete(want, 5, axis=1)).any()
    assert bc.same(bc.lines_numpy(y, k, gamma), want)


@pytest.mark.parametrize("n", [2, 3])
def test_quantile_table_clips_at_three_sigma(n):
    """0.5 -/+ 0.49865: aleph = n q + m leaves [1, n - 1] on both sides, k is clipped and gamma held in [0, 1]."""
    from picaso_amd import retrieval
    q = [bc.LEVELS[4], bc.LEVELS[5]]
    aleph = n * np.array(q) + (0.4 + np.array(q) * 0.2)
    assert aleph[0] < 1 and aleph[1] > n - 1
    k, gamma = retrieval.quantile_table(n, q)
    assert k.tolist() == [1, n - 1] and gamma.tolist() == [0.0, 1.0]
    kk, gg = bc.table_numpy(n, q)
    assert np.array_equal(k, kk) and np.array_equal(gamma, gg)
    x = np.arange(1.0, n + 1)[:, None]
    assert bc.lines_numpy(x, k, gamma).ravel().tolist() == [1.0, float(n)]


def test_quantile_table_other_plotting_positions_and_bad_levels():
    from picaso_amd import retrieval
    q = np.linspace(0, 1, 23)
    for ab in ((0.0, 1.0), (0.5, 0.5), (1.0, 1.0), (0.35, 0.35)):
        k, gamma = retrieval.quantile_table(41, q, *ab)
        kk, gg = bc.table_numpy(41, q, *ab)
        assert np.array_equal(k, kk) and np.array_equal(gamma, gg)
        assert k.min() >= 1 and k.max() <= 40 and gamma.min() >= 0 and gamma.max() <= 1
    assert retrieval.quantile_table(1, [0.1, 0.9])[0].tolist() == [1, 1]
    for bad in ([-0.1], [1.5], [np.nan]):
        with pytest.raises(Exception):
            retrieval.quantile_table(10, bad)
    with pytest.raises(Exception):
        retrieval.quantile_table(0, [0.5])


def _evaluate(retrieval, regrid, model, names=("temperature", "H2O", "CO2")):
    samples = bc.toy_samples()
    np.random.seed(bc.SEED_E)
    return retrieval.get_evaluations(samples, samples[17], model, bc.NDRAWS_E, regrid=regrid, pressure_bands=list(names))


@pytest.mark.parametrize("name", ["newx", "R", "none"])
@pytest.mark.parametrize("frame", [False, True])
def test_get_evaluations_and_chisq_max_equal_the_reference(gold, on_host, name, frame):
    ev = _evaluate(on_host, bc.toy_regrids()[name], bc.toy_model(frame=frame))
    key = "E/%s/" % name
    assert list(ev.keys()) == ["max_logl_ptchem", "bands_spectra", "bands_ptchem", "max_logl_spectra",
                               "max_logl_error_inflation", "max_logl_offsets", "pressure", "wavelength"]
    assert tuple(ev["bands_spectra"].keys()) == bc.KEYS
    assert bc.same(np.stack([ev["bands_spectra"][k] for k in bc.KEYS]), gold[key + "spectra"])
    got = np.stack([[ev["bands_ptchem"][n][k] for k in bc.KEYS] for n in ("temperature", "H2O", "CO2")])
    assert np.array_equal(got, gold[key + "ptchem"])
    assert bc.same(np.asarray(ev["max_logl_spectra"]), gold[key + "max_logl_spectra"])
    assert np.array_equal(ev["wavelength"], gold[key + "wavelength"])
    assert ev["max_logl_error_inflation"] == gold[key + "err"] and ev["max_logl_offsets"]["nirspec"] == gold[key + "offset"]
    assert np.array_equal(np.asarray(ev["pressure"]), gold[key + "pressure"])
    assert np.array_equal(np.asarray(ev["max_logl_ptchem"]["H2O"]), 1e-4 * bc.toy_samples()[17][3] * (1.0 + 0.5 * np.arange(20) / 20.))
    # spectra in one launch, the three profiles in a second one
    assert on_host.calls == [(bc.NDRAWS_E, gold[key + "wavelength"].size), (bc.NDRAWS_E, 3 * bc.NLEVEL_E)]
    chi = on_host.get_chisq_max(ev, bc.toy_data())
    assert sorted(chi) == ["chisq_per_datapt", "datae", "datay", "model", "wavenumber"]
    for k, v in chi.items():
        assert bc.same(np.asarray(v), gold[key + "chisq_" + k]), k


def test_regrid_false_returns_the_unbinned_best_spectrum(on_host):
    """The reference raises NameError here (``binning`` is never set); the bands are on the model's own grid."""
    model = bc.toy_model()
    ev = _evaluate(on_host, False, model)
    x, y, _, _ = model(bc.toy_samples()[17])
    assert np.array_equal(ev["max_logl_spectra"], y) and np.array_equal(ev["wavelength"], 1e4 / x)
    assert ev["bands_spectra"]["median"].shape == (bc.NWNO_E,)


def test_dictionary_of_classes_model(gold, on_host):
    ev = _evaluate(on_host, bc.toy_regrids()["newx"], bc.toy_model(as_dict=True))
    got = np.stack([[ev["bands_ptchem"][n][k] for k in bc.KEYS] for n in ("temperature", "H2O", "CO2")])
    assert np.array_equal(got, gold["E/newx/ptchem"])
    assert np.array_equal(np.asarray(ev["pressure"]), gold["E/newx/pressure"])


def test_no_pressure_bands_skips_the_profile(gold, on_host):
    def model(params, **kw):
        assert not kw, "return_ptchem must not be asked for with pressure_bands=[]"
        return bc.toy_model()(params)
    ev = _evaluate(on_host, bc.toy_regrids()["newx"], model, names=())
    assert sorted(ev) == ["bands_spectra", "max_logl_error_inflation", "max_logl_offsets", "max_logl_spectra", "wavelength"]
    assert bc.same(np.stack([ev["bands_spectra"][k] for k in bc.KEYS]), gold["E/newx/spectra"])
    assert on_host.calls == [(bc.NDRAWS_E, 90)]


def test_subset_of_pressure_bands(gold, on_host):
    ev = _evaluate(on_host, bc.toy_regrids()["newx"], bc.toy_model(), names=("CO2",))
    assert list(ev["bands_ptchem"]) == ["CO2"]
    assert np.array_equal(np.stack([ev["bands_ptchem"]["CO2"][k] for k in bc.KEYS]), gold["E/newx/ptchem"][2])


def test_limits_are_errors_before_any_model_call(on_host):
    def model(*a, **k):
        raise AssertionError("the model must not be evaluated")
    with pytest.raises(Exception, match="16384"):
        on_host.get_evaluations(bc.toy_samples(), bc.toy_samples()[0], model, 16385, pressure_bands=[])
    with pytest.raises(Exception, match="16384"):
        on_host.bands(np.zeros((16385, 2)))
    with pytest.raises(Exception, match="32"):
        on_host.bands(np.zeros((4, 2)), q=np.linspace(0, 1, 33))
    with pytest.raises(Exception):
        on_host.bands(np.zeros(5))


def test_header_declares_the_entry_point_and_its_limits():
    from picaso_amd import _lib, retrieval
    import ctypes
    restype, args = _lib.declared_prototypes()["picaso_column_quantiles_dev"]
    assert restype is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_int,
                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    with open(_lib.HEADER) as fh:
        text = fh.read()
    assert "#define PICASO_BANDS_MAX_DRAWS %d\n" % retrieval.MAX_DRAWS in text
    assert "#define PICASO_BANDS_MAX_Q %d\n" % retrieval.MAX_Q in text


def test_quantile_kernels_compile_for_gfx950_without_spills():
    """hipcc's own resource report for csrc/quantile.hip: three tile sizes, no scratch, the LDS arrays DESIGN 5k names."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import resource_usage
    rows = {r["name"]: r for r in resource_usage.table(os.path.join(root, "picaso_amd", "csrc", "quantile.hip"))}
    kernels = [n for n in rows if "k_column_quantiles" in n]
    assert len(kernels) == 3, sorted(rows)
    for n in kernels:
        r = rows[n]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
        assert r["VGPRs"] <= 32, r
    assert sorted(rows[n]["LDS Size"] for n in kernels) == [16 * 1024, 64 * 1024, 128 * 1024]
