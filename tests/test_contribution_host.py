"""get_contribution / find_press on the host: the public names and signatures of the reference (justdoit.py:1090-1294)."""
import inspect

import numpy as np


def test_get_contribution_signature_matches_the_reference():
    from picaso_amd import justdoit as jdi
    params = inspect.signature(jdi.get_contribution).parameters
    assert list(params) == ["bundle", "opacityclass", "at_tau", "dimension"]
    assert params["at_tau"].default == 1 and params["dimension"].default == "1d"
    assert params["bundle"].default is inspect.Parameter.empty
    assert params["opacityclass"].default is inspect.Parameter.empty


def test_find_press_equals_numpy_interp_per_column_with_ties():
    from picaso_amd import justdoit as jdi
    rng = np.random.default_rng(5)
    nlevel, nwno = 12, 9
    tau = rng.random((nlevel - 1, nwno))
    tau[:5, :4] = 0.0                    # a cloud deck: zero cumulative optical depth above it, ties at 0
    tau[7, 2] = 0.0                      # a tie in the middle of a column
    cum = np.zeros((nlevel, nwno))
    cum[1:] = np.cumsum(tau, axis=0)
    p = np.logspace(-4, 2, nlevel)
    for at_tau in (0.0, 0.5, 1.0, float(cum[8, 2]), 1e3, -1.0, np.nan):
        got = jdi.find_press(at_tau, cum, nwno, p)
        assert isinstance(got, list) and len(got) == nwno
        want = [np.interp(at_tau, cum[:, w], p) for w in range(nwno)]
        np.testing.assert_array_equal(np.array(got), np.array(want))
    assert jdi.find_press(0.0, cum, nwno, p)[0] == p[5]          # the last of the tied levels
