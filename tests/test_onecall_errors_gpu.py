"""onecall.prepare(early=True) puts the opacity stage on the stream (phase 1) before the legs' half of the job is filled: an
exception after that point must reach the caller, hand the block table to ``driver.abandon`` (as ``run`` does after a
failed enqueue) and leave the table fit for the next spectrum, whose results equal those of a fresh opacity object bit for
bit."""
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_devices_gpu import _same
from test_driver_gpu import DB, _case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cloud", [False, True])
def test_error_after_the_opacity_stage_leaves_the_table_usable(monkeypatch, cloud):
    from picaso_amd import driver as drv
    from picaso_amd import justdoit as jdi
    from picaso_amd import onecall
    og = np.load(os.path.join(GOLDEN, "optics.npz"))
    opa = jdi.opannection(filename_db=DB, query_method="linear")
    phases = []
    abandoned = []
    real_enqueue, real_legs, real_abandon = drv.enqueue, onecall._fill_block_legs, drv.abandon

    def enqueue(table, job, phase=0):
        phases.append(phase)
        return real_enqueue(table, job, phase)

    def legs_once(*a, **k):
        if len(phases) == 1:
            raise RuntimeError("injected failure in the legs' half")
        return real_legs(*a, **k)
    def abandon(table):
        abandoned.append(table)
        return real_abandon(table)
    monkeypatch.setattr(drv, "enqueue", enqueue)
    monkeypatch.setattr(drv, "abandon", abandon)
    monkeypatch.setattr(onecall, "_fill_block_legs", legs_once)
    with pytest.raises(RuntimeError, match="injected failure"):
        _case(og, jdi, cloud, True, "none", True).spectrum(opa, calculation="reflected+thermal")
    assert phases == [1]                    # the opacity stage was on the stream when the legs' half raised
    (table,) = opa.__dict__["_driver_tables"].values()
    assert abandoned == [table]             # prepare handed the table back before re-raising
    got = _case(og, jdi, cloud, True, "none", True).spectrum(opa, calculation="reflected+thermal")
    assert phases == [1, 1, 2] and list(opa.__dict__["_driver_tables"].values()) == [table]   # the same table, both phases
    assert abandoned == [table]
    fresh = jdi.opannection(filename_db=DB, query_method="linear")
    _same(_case(og, jdi, cloud, True, "none", True).spectrum(fresh, calculation="reflected+thermal"), got)
