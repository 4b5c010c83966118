"""``picaso_amd.mie`` without a GPU: the Mie series in numpy against 40-digit mpmath and against textbook values, the
``.mieff`` and refractive-index readers, the size distributions and the sum over them against their restatements as loops,
and the reference's two Mie cloud forms (reference picaso/parameterizations.py:59-80, 94-198) step by step."""
import os

import numpy as np
import pytest

from mie_cases import case_list, errors, synthetic_table
from picaso_amd import mie
from picaso_amd import parameterizations as pz
from test_parameterize_host import make_param


def _bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the series
def test_numpy_series_against_mpmath():
    """Every case of the list within 1e-12 of mpmath (dps 40) in the three measures: relative in Qext and Qsca, |delta| /
    Qsca in g Qsca.  Measured here: 1.3e-14 at worst."""
    x, m = case_list()
    assert x.size == 64
    err = errors(mie.mie_efficiencies_numpy(x, m))
    print("mie_efficiencies_numpy vs mpmath: worst Qext %.3g, Qsca %.3g, g %.3g" % tuple(err.max(axis=1)))
    assert err.shape == (3, 64) and np.all(err <= 1e-12), (err.max(axis=1), np.argmax(err, axis=1))


def test_bohren_huffman_point():
    qext, qsca, gq = mie.mie_efficiencies_numpy(2 * np.pi * 0.525 / 0.6328, 1.55)
    assert abs(float(qext) - 3.1054255314658774) <= 1e-13 * 3.1 and abs(float(qsca) - 3.1054255314658774) <= 1e-13 * 3.1
    assert round(float(qext), 5) == 3.10543 and 0 < float(gq) / float(qsca) < 1


@pytest.mark.parametrize("m", [1.33 + 0.0j, 1.5 + 0.02j, 2.2 + 0.7j])
def test_rayleigh_limit(m):
    x = 1e-3
    qext, qsca, _ = (float(v) for v in mie.mie_efficiencies_numpy(x, m))
    K = (m * m - 1) / (m * m + 2)
    assert abs(qsca / ((8.0 / 3.0) * x ** 4 * abs(K) ** 2) - 1) <= 1e-5
    if m.imag:
        assert abs((qext - qsca) / (4 * x * K.imag) - 1) <= 1e-5
    else:
        assert abs(qext - qsca) <= 1e-13 * qsca


def test_no_absorption_means_extinction_is_scattering():
    rng = np.random.default_rng(5)
    x = 10 ** rng.uniform(-4, 2.5, 40)
    m = rng.uniform(1.05, 3, 40) + 0j
    qext, qsca, _ = mie.mie_efficiencies_numpy(x, m)
    assert np.all(np.abs(qext - qsca) <= 1e-13 * qsca)


def test_shapes_and_refused_elements():
    x = np.array([[0.0, 1.0, np.nan], [2.0, -1.0, 0.5]])
    m = np.array([1.5, 1.5 - 0.1j, 1.5])[None, :] + np.zeros((2, 1))
    q = mie.mie_efficiencies_numpy(x, m)
    assert all(a.shape == (2, 3) for a in q)
    assert np.array_equal(np.isnan(q[0]), [[True, True, True], [False, True, False]])
    assert all(np.array_equal(np.isnan(a), np.isnan(q[0])) for a in q)
    one = mie.mie_efficiencies_numpy(2.0, 1.5)
    assert all(_bits(a[1, 0], b) for a, b in zip(q, one))             # an element's value is its own
    assert np.all(np.isnan(mie.mie_efficiencies_numpy(1.0, complex(np.nan, 0.0))[0]))
    with pytest.raises(ValueError, match="at most"):
        mie.mie_efficiencies_numpy(2.0e6, 1.5)
    assert all(a.shape == (0,) for a in mie.mie_efficiencies_numpy(np.zeros(0), 1.5))
    valid, nstop, nmx = mie._orders(np.array([1e-6, 1e3, 0.0]), np.array([1.5, 1.5, 1.5]))
    assert list(nstop) == [2, 1042, 0] and list(valid) == [True, True, False] and nmx[1] == 1606 and nmx[2] == 0


def test_chunks_are_whole_waves_under_the_budget():
    nstop = np.sort(np.r_[np.full(70, 100), np.full(100, 10), np.full(30, 2)])[::-1]         # waves of 100, 100, 10, 2 rows
    row = 3 * 64 * 8
    assert mie._chunks(nstop, 1 << 30) == [(0, 4, 212 * row)]
    assert mie._chunks(nstop, 120 * row) == [(0, 1, 100 * row), (1, 4, 112 * row)]
    assert mie._chunks(nstop, 20 * row) == [(0, 1, 100 * row), (1, 2, 100 * row), (2, 4, 12 * row)]     # a wave over it: alone
    assert mie._chunks(nstop, 0) == [(w, w + 1, r * row) for w, r in enumerate((100, 100, 10, 2))]
    assert mie._chunks(np.array([0, 0]), 0) == [(0, 1, 0)]


# ---- the table and its files
def test_table_rows_are_wavenumber_increasing_whatever_order_they_arrive_in():
    a, b = synthetic_table(), synthetic_table(increasing=True)
    assert np.all(np.diff(a.wavenumber) > 0) and a.wave_in.shape == (7, 4) and a.qext.shape == (7, 4)
    for name in ("qext", "qscat", "cos_qscat", "wave_in", "radius", "area", "wavenumber"):
        assert _bits(getattr(a, name), getattr(b, name)), name
    assert _bits(a.area, mie.PI * a.radius ** 2) and a.digest == b.digest
    qext, qscat, cos_qscat, nwave, radius, wave_in = a
    assert nwave == 7 and qext is a.qext and wave_in is a.wave_in and radius is a.radius
    with pytest.raises(ValueError, match="nwave, nradii"):
        mie.MieTable(a.qext, a.qscat[:, :3], a.cos_qscat, a.radius, a.wave_in)


def test_mieff_round_trip_and_row_order(tmp_path):
    t = synthetic_table()
    mie.write_mieff(str(tmp_path / "SiO2.mieff"), t)
    back = mie.get_mie("SiO2", str(tmp_path))
    for name in ("qext", "qscat", "cos_qscat", "wave_in", "radius"):
        assert _bits(getattr(t, name), getattr(back, name)), name
    lines = open(tmp_path / "SiO2.mieff").read().splitlines()
    assert lines[0].split() == ["7", "4"] and len(lines) == 1 + 4 * 8 and len(lines[1].split()) == 1
    assert float(lines[2].split()[1]) == t.qscat[0, 0] and float(lines[2].split()[2]) == t.qext[0, 0]
    flipped = [lines[0]]
    for i in range(4):                                  # the same file with its rows wavelength increasing
        block = lines[1 + 8 * i:1 + 8 * (i + 1)]
        flipped += [block[0]] + block[:0:-1]
    (tmp_path / "flip.mieff").write_text("\n".join(flipped) + "\n")
    again = mie.get_mie("flip", str(tmp_path))
    for name in ("qext", "qscat", "cos_qscat", "wave_in", "radius"):
        assert _bits(getattr(t, name), getattr(again, name)), name


def test_mieff_reader_refuses_what_does_not_add_up(tmp_path):
    t = synthetic_table()
    mie.write_mieff(str(tmp_path / "a.mieff"), t)
    lines = open(tmp_path / "a.mieff").read().splitlines()
    for name, bad in (("count", ["7 5"] + lines[1:]), ("rows", ["6 4"] + lines[1:]), ("short", lines[:-1]),
                      ("three", lines[:3] + ["1.0 2.0 3.0"] + lines[4:]), ("word", lines[:3] + ["1.0 x 3.0 4.0"] + lines[4:]),
                      ("norad", [lines[0]] + lines[2:]), ("head", ["7"] + lines[1:])):
        (tmp_path / (name + ".mieff")).write_text("\n".join(bad) + "\n")
        with pytest.raises(ValueError, match=name + ".mieff"):
            mie.get_mie(name, str(tmp_path))


def test_read_refrind(tmp_path):
    (tmp_path / "three.refrind").write_text("# wave n k\n0.5 1.5 1e-3\n\n1.0 1.6 2e-3\n")
    (tmp_path / "four.refrind").write_text("1 0.5 1.5 1e-3\n2 1.0 1.6 2e-3\n")
    for name in ("three", "four"):
        w, n, k = mie.read_refrind(str(tmp_path / (name + ".refrind")))
        assert np.array_equal(w, [0.5, 1.0]) and np.array_equal(n, [1.5, 1.6]) and np.array_equal(k, [1e-3, 2e-3])
    (tmp_path / "bad.refrind").write_text("0.5 1.5\n")
    with pytest.raises(ValueError, match="columns"):
        mie.read_refrind(str(tmp_path / "bad.refrind"))


def test_compute_mieff_on_the_host():
    """Sub-radii, default edges and the mean, with the numpy series in the device's place."""
    wave, radius = np.array([0.6, 1.0, 2.5, 5.0, 11.0]), np.array([1e-5, 4e-5, 2e-4])
    nn, kk = np.linspace(1.4, 1.7, 5), np.array([0.0, 1e-4, 1e-2, 0.1, 0.5])
    edges = mie.default_edges(radius)
    assert _bits(edges[1:3], np.sqrt(radius[:-1] * radius[1:])) and abs(edges[0] * edges[1] / radius[0] ** 2 - 1) < 1e-15
    sub = mie.sub_radii(radius, None, 6)
    assert sub.shape == (3, 6) and _bits(sub[:, 0], edges[:-1]) and np.allclose(sub[:, 5], edges[1:], rtol=1e-15)
    assert sub[1, 2] == edges[1] + (edges[2] - edges[1]) * 2 / 5
    t = mie.compute_mieff(wave, nn, kk, radius, efficiencies=mie.mie_efficiencies_numpy)
    assert t.qext.shape == (5, 3) and np.all(np.diff(t.wavenumber) > 0)
    for w in (0, 3):
        for i in (0, 2):
            q = mie.mie_efficiencies_numpy(2 * mie.PI * sub[i] / (wave[w] * 1e-4), complex(nn[w], kk[w]))
            for got, each in zip((t.qext, t.qscat, t.cos_qscat), q):
                acc = each[0]
                for j in range(1, 6):
                    acc = acc + each[j]
                assert got[4 - w, i] == acc / 6
    one = mie.compute_mieff(wave, nn, kk, radius, nsub=1, efficiencies=mie.mie_efficiencies_numpy)
    q = mie.mie_efficiencies_numpy(2 * mie.PI * radius[None, :] / (wave * 1e-4)[:, None], (nn + 1j * kk)[:, None])
    assert _bits(one.qext, q[0][::-1]) and _bits(one.cos_qscat, q[2][::-1])
    with pytest.raises(ValueError, match="edges"):
        mie.compute_mieff(wave, nn, kk, radius, edges_cm=[1e-5, 2e-5])
    with pytest.raises(ValueError, match="neighbours"):
        mie.compute_mieff(wave, nn, kk, radius[:1])


# ---- the sum over a size distribution
def test_particle_distributions_are_the_reference_expressions():
    radius = np.geomspace(1e-5, 3e-3, 9)
    sigma, lograd = 0.37, -3.6
    got = mie.get_particle_dist(radius, "lognormal", lognorm_kwargs={"sigma": sigma, "lograd": lograd})
    logradius = np.log10(radius)
    want = (1 / (sigma * np.sqrt(2 * np.pi)) *
            np.exp(- (logradius - lograd)**2 / (2 * sigma**2)))
    assert _bits(got, want)
    b, lograd = 0.13, -3.2
    got = mie.get_particle_dist(radius, "hansen", hansen_kwargs={"b": b, "lograd": lograd})
    a = 10**lograd
    want = (10**radius)**((1-3*b)/b)*np.exp(-radius/(a*b))
    assert _bits(got, want) and np.all(got > 0)
    with pytest.raises(Exception, match="lognorm_kwargs have not been defined"):
        mie.get_particle_dist(radius, "lognorm")
    with pytest.raises(Exception, match="Only lognormal and hansen"):
        mie.get_particle_dist(radius, "gamma")


def test_calc_optics_user_r_dist_is_three_loops():
    t = synthetic_table(nwave=6, nradii=5)
    qext, qscat, cos_qscat = t.qext.copy(), t.qscat.copy(), t.cos_qscat.copy()
    qext[1], qscat[1] = 0.0, 0.0                        # opd = 0: w0 and g0 are 0, not 0 / 0
    qscat[3], cos_qscat[3] = 0.0, 0.3                   # opd_scat = 0 under opd > 0: g0 is 0
    dist = mie.get_particle_dist(t.radius, "lognorm", {"sigma": 0.5, "lograd": -4.0})
    ndz = 3.7e6
    opd, w0, g0, wno = mie.calc_optics_user_r_dist(t.wave_in, ndz, t.radius, dist, qext, qscat, cos_qscat)
    assert _bits(wno, 1e4 / t.wave_in[:, 0])
    for w in range(6):
        s_ext = s_sca = s_cos = 0.0
        for r in range(5):
            wgt = (ndz * (np.pi * t.radius[r] ** 2)) * dist[r]
            s_ext = s_ext + qext[w, r] * wgt
            s_sca = s_sca + qscat[w, r] * wgt
            s_cos = s_cos + cos_qscat[w, r] * wgt
        assert _bits(opd[w], s_ext), w
        assert _bits(w0[w], s_sca / s_ext if s_ext > 0 else 0.0), w
        assert _bits(g0[w], s_cos / s_sca if s_sca > 0 else 0.0), w
    assert opd[1] == 0 and w0[1] == 0 and g0[1] == 0 and opd[3] > 0 and w0[3] == 0 and g0[3] == 0 and np.all(w0[[0, 2, 4, 5]] > 0)


# ---- the two cloud forms, step by step as reference parameterizations.py:94-198 takes them
LOGNORM = {"sigma": 0.45, "lograd": -3.9}
HANSEN = {"b": 0.17, "lograd": -3.5}


def _format_steps(opd, w0, g0, pressure, inside, scaled):
    """picaso_format's table (reference :672-750) element by element: ``(opd, w0, g0)`` columns, layer by layer."""
    cols = ([], [], [])
    for l in range(len(pressure)):
        for w in range(len(opd)):
            vals = (scaled(l, w), w0[w], g0[w]) if inside[l] else (opd[w] * 0, w0[w] * 0, g0[w] * 0)
            for c, v in zip(cols, vals):
                c.append(v)
    return [np.array(c) for c in cols]


@pytest.mark.parametrize("distribution,decay", [("lognorm", "slab"), ("hansen", "deck")])
def test_cloud_brewster_mie_step_by_step(distribution, decay):
    p, t = make_param(5), synthetic_table()
    slab = {"ptop": float(np.log10(p.pressure_layer[1])), "dp": 1.1, "reference_tau": 2.5}
    deck = {"ptop": float(np.log10(p.pressure_layer[2])), "dp": 0.4}
    df = mie.cloud_brewster_mie(p, t, distribution, decay, lognorm_kwargs=LOGNORM, hansen_kwargs=HANSEN, slab_kwargs=slab,
                                deck_kwargs=deck)
    dist = mie.get_particle_dist(t.radius, distribution, LOGNORM, HANSEN)
    opd, w0, g0, grid = mie.calc_optics_user_r_dist(t.wave_in, 1, t.radius, dist, t.qext, t.qscat, t.cos_qscat)
    profile = p.slab_decay(**slab) if decay == "slab" else p.deck_decay(**deck)
    top = max(opd)
    want = _format_steps(opd, w0, g0, p.pressure_layer, [True] * 5, lambda l, w: profile[l] * (opd[w] / top))
    assert list(df.columns) == ["pressure", "wavenumber", "opd", "w0", "g0"] and len(df) == 5 * 7
    for name, col in zip(("opd", "w0", "g0"), want):
        assert _bits(df[name].values, col), name
    assert _bits(df["wavenumber"].values, np.tile(grid, 5)) and _bits(df["pressure"].values, np.repeat(p.pressure_layer, 7))
    assert np.any(df["opd"].values > 0) and np.all(np.diff(grid) > 0)
    with pytest.raises(Exception, match="decay_type"):
        mie.cloud_brewster_mie(p, t, distribution, "box", LOGNORM, HANSEN)


@pytest.mark.parametrize("distribution,base", [("lognorm", 0.3), ("hansen", 1e3), ("lognorm", 1e-9)])
def test_cloud_flex_fsed_step_by_step(distribution, base):
    p, t = make_param(5), synthetic_table()
    base = base if base != 0.3 else float(p.pressure_layer[2]) * 1.0001
    ndz, fsed = 2.5e7, 1.7
    df = mie.cloud_flex_fsed(p, t, base, ndz, fsed, distribution, lognorm_kwargs=LOGNORM, hansen_kwargs=HANSEN)
    assert mie.flex_cloud is mie.cloud_flex_fsed
    dist = mie.get_particle_dist(t.radius, distribution, LOGNORM, HANSEN)
    opd, w0, g0, grid = mie.calc_optics_user_r_dist(t.wave_in, ndz, t.radius, dist, t.qext, t.qscat, t.cos_qscat)
    pl = p.pressure_layer
    z = np.linspace(100, 0, 5)
    opd_h = [10.0 * np.exp(-fsed * z[l] / 10) if base >= pl[l] else 0.0 for l in range(5)]
    with np.errstate(invalid="ignore"):
        opd_h = [np.float64(v) / max(opd_h) for v in opd_h]
        decay = [v / np.max(opd_h) for v in opd_h]
    inside = [1e-10 <= pl[l] <= base for l in range(5)]
    want = _format_steps(opd, w0, g0, pl, inside, lambda l, w: decay[l] * opd[w])
    for name, col in zip(("opd", "w0", "g0"), want):
        assert _bits(df[name].values, col), name
    if base < pl[0]:
        assert not np.any(df["opd"].values) and not np.any(df["w0"].values)     # the base above every layer: nothing anywhere
        avg = pz.cloud_averaging([df])
        assert np.all(avg["opd"].values == 1e-33)
    else:
        assert np.any(df["opd"].values > 0) and (base > pl[-1] or np.any(df["opd"].values.reshape(5, 7)[-1] == 0))


def test_batch_records_are_the_per_sample_values():
    """The host half of ``cloud_tables_batch`` (no GPU): weights, layer factors and masks formed for the whole batch at once
    equal what the per-sample functions form, bit for bit."""
    p, t, t2 = make_param(5), synthetic_table(), synthetic_table(nradii=1, seed=4)
    pl = p.pressure_layer
    slab = {"ptop": float(np.log10(pl[1])), "dp": 1.1, "reference_tau": 2.5}
    samples = [[dict(kind="brewster_mie", table=t, distribution="hansen", decay_type="slab", hansen_kwargs=HANSEN, slab_kwargs=slab),
                dict(kind="flex_fsed", table=t2, distribution="lognorm", base_pressure=float(pl[3]), ndz=4e6, fsed=0.8,
                     lognorm_kwargs=LOGNORM)],
               [dict(kind="flex_fsed", table=t, distribution="hansen", base_pressure=1e-9, ndz=1e5, fsed=2.0, hansen_kwargs=HANSEN)]]
    tables, deck_table, deck_kind, wgt, factor, inside, average, stamps = mie._batch_records(p, samples)
    assert tables == [t, t2] and deck_table.tolist() == [[0, 1], [0, -1]] and deck_kind.tolist()[0] == [0, 1] and average == 1
    assert wgt.shape == (2, 2, 4) and len(stamps) == 2 and len(stamps[0]) == 2
    assert _bits(wgt[0, 0], (1 * t.area) * mie.get_particle_dist(t.radius, "hansen", hansen_kwargs=HANSEN))
    assert _bits(wgt[0, 1, :1], (4e6 * t2.area) * mie.get_particle_dist(t2.radius, "lognorm", LOGNORM)) and not np.any(wgt[0, 1, 1:])
    assert _bits(wgt[1, 0], (1e5 * t.area) * mie.get_particle_dist(t.radius, "hansen", hansen_kwargs=HANSEN))
    assert _bits(factor[0, 0], p.slab_decay(**slab)) and np.all(inside[0, 0] == 1)
    decay = mie._fsed_decay(pl, float(pl[3]), 0.8)
    assert _bits(factor[0, 1], decay / np.max(decay)) and inside[0, 1].tolist() == [1, 1, 1, 1, 0]
    assert np.all(np.isnan(factor[1, 0])) and not np.any(inside[1, 0]) and not np.any(inside[1, 1])
    with pytest.raises(ValueError, match="1 to 4 decks"):
        mie._batch_records(p, [[]])
    with pytest.raises(ValueError, match="one wavelength grid"):
        mie._batch_records(p, [[dict(samples[1][0], table=synthetic_table(nwave=6))], samples[1]])
    with pytest.raises(Exception, match="brewster_mie"):
        mie._batch_records(p, [[dict(samples[1][0], kind="brewster_grey")]])


def test_the_refusals_name_the_functions_that_do_the_job():
    p = make_param(5)
    for fn, word in (("cloud_flex_fsed", "mie.cloud_flex_fsed"), ("flex_cloud", "mie.cloud_flex_fsed"),
                     ("cloud_brewster_mie", "mie.cloud_brewster_mie"), ("cloud_virga", "mie.cloud_flex_fsed")):
        with pytest.raises(NotImplementedError, match=word):
            getattr(p, fn)()
    with pytest.raises(NotImplementedError, match="mie.get_mie"):
        pz.Parameterize(mieff_dir=os.sep)
