"""The one-call driver's block tables (``onecall._block_table``) are keyed on what a table holds -- the planes written and
what the legs read -- not on per-call job fields: SH spectra whose cloud decks begin at different layers (``sh_top``, a
field of the job) share one table, and each equals the call-by-call path bit for bit."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_devices_gpu import _same
from test_driver_gpu import DB, _case

pytestmark = pytest.mark.gpu


def test_sh_cloud_decks_share_one_block_table(monkeypatch):
    from picaso_amd import justdoit as jdi
    og = np.load(os.path.join(GOLDEN, "optics.npz"))
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    nlayer = og["in/cld_opd"].shape[0]

    def make(deck):
        cld = {k: np.array(og["in/cld_" + k]) for k in ("opd", "w0", "g0")}
        cld["opd"] = np.abs(cld["opd"]) + 0.05
        for k in ("opd", "g0"):
            cld[k][:deck] = 0.0
        c = _case(og, jdi, True, True, "none", True)
        c.approx(raman="none", delta_eddington=True, rt_method="SH", stream=4)
        c.clouds(df=cld)
        assert jdi._cloud_free_top(c.inputs, nlayer) == deck
        return c
    decks = (3, nlayer // 2, nlayer - 5)
    got = [make(d).spectrum(opa, calculation="reflected+thermal") for d in decks]
    assert len(opa.__dict__["_driver_tables"]) == 1
    monkeypatch.setenv("PICASO_AMD_NO_DRIVER", "1")
    for d, g in zip(decks, got):
        _same(make(d).spectrum(opa, calculation="reflected+thermal"), g)
