"""The guessed bracket of csrc/interp.hpp (``regrid_bracket_guess``) through both kernels that use it, bit for bit against
numpy: ``picaso_xsec_resample_dev`` is ``np.interp(x, xp, fp, left, right)`` and a floor, ``picaso_xsec_axpy_dev`` with
``first = 1, weight = 1.0`` is ``0.0 + np.interp(x, xp, fp)``.  The guess ``(start, step)`` only says where to look first:
whatever it is -- exact, a few knots off (the walk corrects it), far off or not a number (the binary search takes over) --
the index is numpy's, so every case asserts equal bits."""
import numpy as np
import pytest

from picaso_amd import _lib
from picaso_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

LEFT, RIGHT, FLOOR = 3.0, 5.0, -0.5                 # distinct, and both fills above the floor: a side mix-up shows
N_OUT = (1, 64, 65, 1000)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def uniform_grid():
    return np.arange(257) * 0.37 + 1234.5


def nonuniform_grid():
    xp = 1000.0 * np.sort(np.random.default_rng(5).uniform(size=300) ** 3)
    for k in (50, 150, 250):                        # three pairs of equal neighbouring knots
        xp[k + 1] = xp[k]
    assert np.all(xp[1:] >= xp[:-1]) and np.sum(xp[1:] == xp[:-1]) == 3
    return xp


def span_guess(xp):
    """what the host gives the kernels: the first knot and the step of a uniform grid of this span"""
    return float(xp[0]), (float(xp[-1]) - float(xp[0])) / (xp.size - 1)


def uniform_guesses(xp):
    start, step = span_guess(xp)
    inf, nan = float("inf"), float("nan")
    g = [("exact", start, step)]
    g += [("start %+d knots" % k, start + k * step, step) for k in (-3, 3, -5, 5, -100, 100)]     # walk; then the search
    g += [("step x 0.5", start, 0.5 * step), ("step x 3", start, 3.0 * step)]
    g += [("step %r" % s, start, s) for s in (0.0, -step, inf, nan)]
    g += [("start %r" % s, s, step) for s in (inf, nan)]
    return g


def abscissae(xp, n_out, rng):
    """``n_out`` points: below and above the grid, on its first and last knot, on interior knots and on a tied one (the
    grid's own, else another interior knot), strictly inside brackets, and one NaN, in shuffled order.  ``n_out = 1``: the
    eight kinds, one array each."""
    ties = np.nonzero(xp[1:] == xp[:-1])[0]
    inner = xp[1:-1] if xp.size > 2 else xp
    mid = 0.5 * (xp[:-1] + xp[1:])
    mid = mid[(mid > xp[:-1]) & (mid < xp[1:])]
    kinds = [xp[0] - 1.0, xp[-1] + 1.0, xp[0], xp[-1], inner[inner.size // 3], xp[ties[0]] if ties.size else inner[-1],
             mid[mid.size // 2], np.nan]
    if n_out == 1:
        return [np.array([v]) for v in kinds]
    span = xp[-1] - xp[0]
    x = np.concatenate((kinds, rng.choice(inner, n_out // 4), rng.choice(mid, n_out // 4),
                        rng.uniform(xp[0] - 0.05 * span, xp[-1] + 0.05 * span, n_out)))[:n_out]
    rng.shuffle(x)
    assert np.isnan(x).sum() == 1 and (x < xp[0]).any() and (x > xp[-1]).any() and np.isin(x, xp).sum() >= 6
    return [x]


def check(xp, guesses, n_out):
    ctx, lib = _lib.context(), _lib.load()
    rng = np.random.default_rng(1000 + n_out + xp.size)
    fp = rng.uniform(-1.0, 1.0, xp.size)
    d_xp, d_fp = DeviceArray.from_host(xp, ctx), DeviceArray.from_host(fp, ctx)
    try:
        for x in abscissae(xp, n_out, rng):
            with np.errstate(invalid="ignore"):
                want_r = np.interp(x, xp, fp, LEFT, RIGHT)
                want_r[want_r < FLOOR] = FLOOR
                want_a = 0.0 + np.interp(x, xp, fp)
            d_x, d_out = DeviceArray.from_host(x, ctx), DeviceArray.from_host(np.full(x.size, 99.0), ctx)
            try:
                for name, start, step in guesses:
                    _lib.check(lib.picaso_xsec_resample_dev(ctx, x.size, d_out.addr, d_fp.addr, xp.size, d_xp.addr, d_x.addr,
                                                            start, step, LEFT, RIGHT, FLOOR), ctx)
                    got = d_out.to_host()
                    bad = np.nonzero(bits(got) != bits(want_r))[0]
                    assert bad.size == 0, ("resample", name, bad[:5], x[bad[:5]], got[bad[:5]], want_r[bad[:5]])
                    _lib.check(lib.picaso_xsec_axpy_dev(ctx, x.size, d_out.addr, 1, 1.0, d_fp.addr, xp.size, d_xp.addr,
                                                        d_x.addr, start, step), ctx)
                    got = d_out.to_host()
                    bad = np.nonzero(bits(got) != bits(want_a))[0]
                    assert bad.size == 0, ("axpy", name, bad[:5], x[bad[:5]], got[bad[:5]], want_a[bad[:5]])
            finally:
                d_x.free()
                d_out.free()
    finally:
        d_xp.free()
        d_fp.free()


@pytest.mark.parametrize("n_out", N_OUT)
def test_uniform_grid_under_every_guess(n_out):
    xp = uniform_grid()
    assert xp.size == 257
    check(xp, uniform_guesses(xp), n_out)


@pytest.mark.parametrize("n_out", N_OUT)
def test_two_knots(n_out):
    xp = np.array([10.0, 20.0])
    check(xp, [("exact",) + span_guess(xp), ("step 0", 10.0, 0.0)], n_out)


@pytest.mark.parametrize("n_out", N_OUT)
def test_nonuniform_grid_with_tied_knots(n_out):
    xp = nonuniform_grid()
    check(xp, [("the guess of its span",) + span_guess(xp), ("step 0", float(xp[0]), 0.0)], n_out)
