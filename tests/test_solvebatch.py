"""``solvebatch.SolveBatch``: which records share a launch, which wrapper each launch goes through and in what order.
The ``resident`` wrappers are replaced by a recorder: no GPU, no library."""
import numpy as np
import pytest

from picaso_amd import solvebatch
from picaso_amd.solvebatch import Reflected1D, Reflected3D, Solve, SolveBatch, Thermal1D, Thermal3D

TTHG = (3, 1, 0.11, 0.22, 0.33, 0.44, 0.55)
NLEVEL, NWNO = 7, 13


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs))
        return call


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(solvebatch, "resident", r)
    return r


def _weights(ng, nt):
    return tuple(np.full(ng, 1.0 / ng)), tuple(np.full(nt, 1.0 / nt))


def reflected_1d(tag, ng=3, nt=2, cos_theta=0.7, shift=0.0, b_top=0.0, present=("dtau", "w0"), lvl=None, ctx="ctx"):
    u0 = 0.1 + np.arange(ng * nt, dtype=float).reshape(ng, nt) / 40 + shift
    key = Reflected1D(NLEVEL, NWNO, ng, nt, TTHG, 0, b_top, *_weights(ng, nt), present)
    return Solve("reflected_1d", ctx, key, dict(planes={"dtau": tag}, rs="rs" + tag, ubar0=u0, ubar1=u0 + 0.01,
                                                cos_theta=cos_theta, F0PI="f0" + tag, xint="x" + tag, albedo="alb" + tag,
                                                lvl=lvl))


def thermal_1d(tag, ng=3, nt=2, shift=0.0, wno=1000, disk=True, lvl=None, options=None):
    key = Thermal1D(NLEVEL, NWNO, ng, nt, 1, wno, *_weights(ng, nt))
    u1 = 0.1 + np.arange(ng * nt, dtype=float).reshape(ng, nt) / 40 + shift
    return Solve("thermal_1d", "tctx", key,
                 dict(wno="wno", tlevel=np.full(NLEVEL, 500.0), plevel=np.full(NLEVEL, 2.0), dtau="dt" + tag, w0="w0" + tag,
                      cosb="cb" + tag, ubar1=u1, rs="rs" + tag, flux="fx" + tag, disk="disk" + tag if disk else None, lvl=lvl,
                      options=options or {}))


def reflected_3d(tag, fm=False, ng=3, nt=2):
    key = Reflected3D(NLEVEL, NWNO, ng, nt, TTHG, ("dtau", "w0"), fm, *_weights(ng, nt))
    u0 = np.full((ng, nt), 0.5)
    return Solve("reflected_3d", "ctx", key, dict(planes={"dtau": tag}, rs="rs" + tag, ubar0=u0, ubar1=u0, cos_theta=0.7,
                                                  F0PI="f0" + tag, xint="x" + tag, albedo="alb" + tag))


def thermal_3d(tag, fm=False, has_cosb=True, ng=3, nt=2):
    key = Thermal3D(NLEVEL, NWNO, ng, nt, 0, 1000, has_cosb, fm, *_weights(ng, nt))
    return Solve("thermal_3d", "ctx", key,
                 dict(wno="wno", tlevel=np.full((NLEVEL, ng, nt), 500.0), plevel=np.full((NLEVEL, ng, nt), 2.0), dtau="dt" + tag,
                      w0="w0" + tag, cosb="cb" + tag if has_cosb else None, ubar1=np.full((ng, nt), 0.5), rs="rs" + tag,
                      flux="fx" + tag, disk="disk" + tag), keep={"dtau": tag})


def _flush(*solves):
    batch = SolveBatch()
    for s in solves:
        batch.add(s)
    assert batch.pending() == len(solves)
    batch.flush()
    assert batch.pending() == 0
    return batch


def test_records_with_different_keys_never_share_a_launch(rec):
    """Among them the two members that are no argument of a launch: the present planes and the wavenumber grid."""
    _flush(reflected_1d("a"), reflected_1d("b"), reflected_1d("c", b_top=0.5), reflected_1d("d", present=("dtau",)),
           thermal_1d("a"), thermal_1d("b"), thermal_1d("c", wno=2000))
    assert [c[0] for c in rec.calls] == ["reflected_1d_batch", "reflected_1d", "reflected_1d", "thermal_1d_batch", "thermal_1d"]
    assert [pl["dtau"] for pl in rec.calls[0][1][5]] == ["a", "b"]
    assert rec.calls[1][1][5] == {"dtau": "c"} and rec.calls[1][2]["b_top"] == 0.5
    assert rec.calls[2][1][5] == {"dtau": "d"}
    assert rec.calls[3][1][7] == ["dta", "dtb"] and rec.calls[4][1][7] == "dtc"


def test_single_member_and_wide_disk_go_alone_through_the_plain_wrapper(rec):
    one = reflected_1d("a")
    wide = [reflected_1d(t, ng=6, nt=2) for t in "bc"] + [thermal_1d(t, ng=6, nt=2) for t in "bc"]
    _flush(one, thermal_1d("a"), *wide)
    assert [c[0] for c in rec.calls] == ["reflected_1d"] * 3 + ["thermal_1d"] * 3
    name, args, kw = rec.calls[0]
    k, a = one.key, one.args
    assert args == ("ctx", NLEVEL, NWNO, 3, 2, a["planes"], "rsa", a["ubar0"], a["ubar1"], 0.7, "f0a", *TTHG, "xa")
    assert kw == dict(toon_coefficients=0, b_top=0.0, gweight=k.gweight, tweight=k.tweight, albedo="alba", lvl_fluxes=None)
    name, args, kw = rec.calls[3]
    assert args[:6] == ("tctx", NLEVEL, "wno", NWNO, 3, 2) and args[7:10] == ("dta", "w0a", "cba") and args[12:] == ("rsa", 1, "fxa")
    assert kw == dict(gweight=_weights(3, 2)[0], tweight=_weights(3, 2)[1], flux_disk="diska", lvl_fluxes=None)


def test_launch_alone_carries_level_fluxes_and_unfused_options(rec):
    """What ``Spectrum`` launches without a batch: the plain wrapper, with the level fluxes and without the disk sum."""
    unfused = reflected_1d("a", lvl=["l0", "l1", "l2", "l3"])
    unfused.args["albedo"] = None
    solvebatch.launch(unfused)
    solvebatch.launch(thermal_1d("a", disk=False, lvl=["t0", "t1", "t2", "t3"], options=dict(dwno="dw", calc_type=1)))
    (n0, _, kw0), (n1, _, kw1) = rec.calls
    assert (n0, n1) == ("reflected_1d", "thermal_1d")
    assert kw0["lvl_fluxes"] == ["l0", "l1", "l2", "l3"] and kw0["albedo"] is None and kw0["gweight"] is not None
    assert kw1 == dict(lvl_fluxes=["t0", "t1", "t2", "t3"], dwno="dw", calc_type=1)


def test_equal_geometry_collapses_and_one_differing_cos_theta_does_not(rec):
    same = [reflected_1d(t) for t in "abc"]
    _flush(*same, *[thermal_1d(t) for t in "abc"])
    (name, args, kw), (tname, targs, _) = rec.calls
    assert (name, tname) == ("reflected_1d_batch", "thermal_1d_batch")
    assert args[7].shape == (3, 2) and args[8].shape == (3, 2) and np.ndim(args[9]) == 0 and args[9] == 0.7
    assert targs[11].shape == (3, 2) and targs[6].shape == (3, NLEVEL) and targs[10].shape == (3, NLEVEL)
    assert kw["albedo"] == ["alba", "albb", "albc"] and args[6] == ["rsa", "rsb", "rsc"]
    del rec.calls[:]
    _flush(reflected_1d("a"), reflected_1d("b", cos_theta=0.6), reflected_1d("c"),
           thermal_1d("a"), thermal_1d("b", shift=0.01), thermal_1d("c"))
    (name, args, _), (tname, targs, _) = rec.calls
    assert (name, tname) == ("reflected_1d_batch", "thermal_1d_batch")
    assert args[7].shape == (3, 3, 2) and args[8].shape == (3, 3, 2)
    assert np.array_equal(args[9], [0.7, 0.6, 0.7])
    assert targs[11].shape == (3, 3, 2) and targs[11][1, 0, 0] == pytest.approx(0.11)


def test_3d_group_of_one_goes_through_the_batch_wrapper(rec):
    _flush(reflected_3d("a"), thermal_3d("a", has_cosb=False))
    (name, args, kw), (tname, targs, tkw) = rec.calls
    assert (name, tname) == ("reflected_3d_batch", "thermal_3d_batch")
    assert args[5] == [{"dtau": "a"}] and args[7].shape == (1, 3, 2) and np.array_equal(args[9], [0.7])
    assert kw["albedo"] == ["alba"]
    assert targs[6].shape == (1, NLEVEL, 3, 2) and targs[7] == ["dta"] and targs[9] is None and tkw["flux_disk"] == ["diska"]


def test_facet_major_planes_select_the_fm_wrappers(rec):
    _flush(reflected_3d("a", fm=True), reflected_3d("b", fm=True), reflected_3d("c"), thermal_3d("a", fm=True), thermal_3d("c"))
    assert [c[0] for c in rec.calls] == ["reflected_3d_fm_batch", "reflected_3d_batch", "thermal_3d_fm_batch",
                                         "thermal_3d_batch"]
    assert rec.calls[2][1][9] == ["cba"]
    del rec.calls[:]
    # without a batch: facet-major planes go through the fm batch of one, the others through the plain wrappers
    for s in (reflected_3d("a", fm=True), reflected_3d("c"), thermal_3d("a", fm=True), thermal_3d("c")):
        solvebatch.launch(s)
    assert [c[0] for c in rec.calls] == ["reflected_3d_fm_batch", "reflected_3d", "thermal_3d_fm_batch", "thermal_3d"]
    assert rec.calls[1][1][5] == {"dtau": "c"} and rec.calls[1][1][-1] == "albc"
    assert rec.calls[3][1][6].shape == (NLEVEL, 3, 2) and rec.calls[3][1][-1] == "diskc"


def test_pending_counts_all_legs_and_flush_order(rec):
    """3-D before 1-D, reflected before thermal, groups in the order they were first added."""
    batch = SolveBatch()
    for s in (thermal_1d("a"), thermal_1d("b"), reflected_1d("a", b_top=0.5), reflected_1d("a"), reflected_1d("b"),
              thermal_3d("a"), reflected_3d("a"), reflected_1d("c", b_top=0.5)):
        batch.add(s)
    assert batch.pending() == 8
    batch.flush()
    assert batch.pending() == 0
    assert [c[0] for c in rec.calls] == ["reflected_3d_batch", "thermal_3d_batch", "reflected_1d_batch", "reflected_1d_batch",
                                         "thermal_1d_batch"]
    assert rec.calls[2][2]["b_top"] == 0.5 and rec.calls[3][2]["b_top"] == 0.0
    batch.flush()
    assert len(rec.calls) == 5
