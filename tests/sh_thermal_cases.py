"""Shared by test_oracle_golden.py (CPU) and test_fuzz_gpu.py / test_sh_thermal_gpu.py (GPU): the seeded random draws
and the hand-made edge inputs of get_thermal_SH, so that the check "the fp64 oracle is within 1e-9 of its x87 build on
this input" and the check "the kernel agrees with the oracle on this input" see the same arrays.

A draw is ``(args, tag)``: ``args`` the positional arguments of ``fluxes.get_thermal_SH`` / ``oracle.get_thermal_SH``."""
import functools
import os

import numpy as np

OFFSET = int(os.environ.get("PICASO_FUZZ_OFFSET", "0"))        # shifts every seed, as in test_fuzz_gpu.py
NBLOCK, NDRAW = 4, 16
SH_MAX_ANG = 16                                                 # sh.hpp: angles of one launch of k_sh_thermal

# Offset 0 is the committed set: every block must hold at least three draws with more than SH_MAX_ANG angles (a second
# launch of launch_sh_thermal) and one with 17 or 18 (a short second launch).  The recipe gives 5 x 4, 6 x 3 or 6 x 4 to about
# one draw in eight, so some blocks get there by themselves (block 2 does) and others do not; rather than depend on which,
# three draws of every block have their geometry set by hand -- (block, draw) -> (ng, nt, phase) -- after everything else
# has been drawn, so the generator's stream is not disturbed and an edit of the recipe cannot lose the coverage:
GEOMETRY_BY_HAND = {
    (0, 2): (6, 3, 0.4), (0, 7): (5, 4, 1.1), (0, 12): (6, 4, 0.0),
    (1, 1): (6, 3, 2.0), (1, 6): (6, 4, 0.4), (1, 11): (5, 4, 0.0),
    (2, 3): (6, 3, 0.0), (2, 8): (5, 4, 2.0), (2, 13): (6, 4, 1.1),
    (3, 0): (6, 3, 1.1), (3, 5): (6, 4, 2.0), (3, 10): (5, 4, 0.4),
}


def geometry(ng, nt, phase=0.0):
    """ubar1 (ng, nt), gweight, tweight: the 1-D Gauss table for nt = 1, else the ng x nt grid at ``phase``."""
    from picaso_amd import disco
    if nt == 1:
        g, gw, t, tw = disco.get_angles_1d(ng)
    else:
        g, gw, t, tw = disco.get_angles_3d(ng, nt)
    _, u1, _, _, _ = disco.compute_disco(ng, nt, g, t, phase)
    return np.ascontiguousarray(u1, dtype=np.float64), np.asarray(gw, dtype=np.float64), np.asarray(tw, dtype=np.float64)


def sh_args(sc, ng, nt, u1, rs, stream, hard, delta=True):
    """``delta``: cosb is the delta-scaled plane (the reference then forms ff = cosb_og**stream), else cosb_og itself
    (its np.array_equal test holds and ff = 0; fluxes.py:3072-3075)."""
    nlayer, nwno = sc["dtau"].shape
    cosb = sc["cosb"] if delta else sc["cosb_og"]
    return (nlayer + 1, sc["wno"], nwno, ng, nt, sc["tlevel"], sc["dtau"], sc["tau"], sc["w0"], cosb, sc["dtau_og"],
            sc["tau_og"], sc["w0_og"], sc["w0_no_raman"], sc["cosb_og"], sc["plevel"], u1, rs, stream, hard)


@functools.lru_cache(maxsize=None)
def block_draws(block, offset=OFFSET):
    """The NDRAW draws of a block, all from one generator."""
    from picaso_amd import synthetic as syn
    rng = np.random.default_rng(5000 + block + 7919 * offset)
    out = []
    for it in range(NDRAW):
        nlayer = int(rng.choice([1, 2, 3, 7, 19, 40, 90]))
        nwno = int(rng.choice([1, 5, 63, 64, 65, 130, 255, 256, 257, 300]))
        stream = int(rng.choice([2, 4]))
        hard = int(rng.integers(0, 2))
        delta = bool(rng.integers(0, 2))
        kw = dict(delta_eddington=bool(rng.integers(0, 2)))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            kw.update(cloud=False)
        elif kind == 1:
            kw.update(cloud_opd=float(10.0 ** rng.uniform(-2, 1.5)))
        elif kind == 2:
            kw.update(gas_scale=float(10.0 ** rng.uniform(-3, 2)), ray_scale=float(10.0 ** rng.uniform(-1, 1)))
        rs = float(rng.choice([0.0, 0.2])) if rng.random() < 0.6 else 0.5 * rng.random(nwno)
        if rng.random() < 0.4:
            ng, nt, phase = int(rng.choice([5, 6, 7, 8])), 1, 0.0
        else:
            ng, nt = int(rng.integers(2, 7)), int(rng.integers(2, 5))
            phase = float(rng.choice([0.0, 0.4, 1.1, 2.0]))
        if offset == 0:
            ng, nt, phase = GEOMETRY_BY_HAND.get((block, it), (ng, nt, phase))
        sc = syn.make_scene(nlayer, nwno, seed=5000 + 64 * offset + NDRAW * block + it, stream=stream, **kw)
        u1, _, _ = geometry(ng, nt, phase)
        tag = (block, it, nlayer, nwno, ng, nt, stream, hard, int(delta), int(kw["delta_eddington"]), kind)
        out.append((sh_args(sc, ng, nt, u1, rs, stream, hard, delta), tag))
    return out


def draw(block, it, offset=OFFSET):
    return block_draws(block, offset)[it]


def w0max(args):
    return float(np.max(args[8]))


def reaches_clip(args):
    """Some column and angle has (1/u1 + lambda) dtau > 35 in some layer: the kernel then leaves the product of two
    exponentials for exponentials of the clipped arguments (the `!noclip` branch of k_sh_thermal).  lambda >= 0, so
    dtau / u1 > 35 is sufficient."""
    return bool(np.max(args[6]) / np.min(args[16]) > 35.0)


# ---- deterministic edges ----
def planck_overflow(stream, hard):
    """25 K at the top and wavenumbers up to 33 000 cm^-1: hc wno / kT reaches 1 900, the exponential of the Planck function
    overflows and the reference forms 1 / (inf - 1) = 0 for the cold levels of the blue columns (fluxes.py:1660-1680)."""
    from picaso_amd import synthetic as syn
    nlayer, nwno = 7, 65
    sc = dict(syn.make_scene(nlayer, nwno, seed=77, stream=stream))
    sc["wno"] = np.linspace(300.0, 33000.0, nwno)
    sc["tlevel"] = np.linspace(25.0, 400.0, nlayer + 1)
    u1, _, _ = geometry(5, 1)
    return sh_args(sc, 5, 1, u1, 0.1, stream, hard)


def _sh_lambdas(w0, stream):
    """Eigenvalues of a cloud-free layer (cosb_og = 0: Legendre weights (1, 0, 0, 0), a_l = (1 - w0, 3, 5, 7)):
    fluxes.py:3245-3251 (SH2), :3388-3400 (SH4)."""
    a0, a1, a2, a3 = 1.0 - w0, 3.0, 5.0, 7.0
    if stream == 2:
        return (np.sqrt(a0 * a1),)
    beta = a0 * a1 + 4 * a0 * a3 / 9 + a2 * a3 / 9
    gama = a0 * a1 * a2 * a3 / 9
    disc = np.sqrt(beta * beta - 4 * gama)
    return np.sqrt((beta + disc) / 2), np.sqrt((beta - disc) / 2)


def resonant_w0(stream, root, target):
    """w0 in (0, 1) with eigenvalue ``root`` equal to ``target``, by bisection (the eigenvalues fall as w0 grows); None
    where no such w0 exists."""
    lo, hi = 1e-6, 1.0 - 1e-6
    f = lambda w: _sh_lambdas(w, stream)[root] - target
    if not (f(lo) > 0.0 > f(hi)):
        return None
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid) > 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


RESONANCE_D = (1e-3, 1e-5, 1e-7)
RESONANCE_LAYER = 3


@functools.lru_cache(maxsize=None)
def resonance_cases(stream):
    """[(root, angle index, d, args)]: a cloud-free 7 x 64 scene on the 5-point Gauss table whose layer RESONANCE_LAYER has
    eigenvalue ``root`` at (1 / u1)(1 + d) for table angle ``angle index`` -- next to the singularity 1 / (1/u1 - lambda) of
    the source-function integral (fluxes.py:3116-3119, :3133-3140) -- for every root and table angle that admit a w0 in
    (0, 1) and every d of RESONANCE_D.  d = 0 is no case: the reference divides by zero there."""
    from picaso_amd import synthetic as syn
    nlayer, nwno = 7, 64
    u1, _, _ = geometry(5, 1)
    base = syn.make_scene(nlayer, nwno, seed=78, stream=stream, cloud=False)
    out = []
    for root in range(stream // 2):
        for k, u in enumerate(u1.ravel()):
            for d in RESONANCE_D:
                w = resonant_w0(stream, root, (1.0 / u) * (1.0 + d))
                if w is None:
                    continue
                sc = dict(base)
                # cloud-free: the delta-scaling is the identity and w0, w0_og, w0_no_raman are the same plane up to the
                # Raman factor; the solver reads w0
                for key in ("w0", "w0_og", "w0_no_raman"):
                    sc[key] = base[key].copy()
                    sc[key][RESONANCE_LAYER, :] = w
                out.append((root, k, d, sh_args(sc, 5, 1, u1, 0.0, stream, 0)))
    return out
