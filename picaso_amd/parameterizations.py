"""Parameter vector -> T(P) profile, abundance table, cloud table: what every ``model(cube)`` of a free retrieval calls
(reference picaso/parameterizations.py, class ``Parameterize``), with the reference's call surface and returns.

The T(P) and chemistry forms and the cloud profile shapes are host code on a few dozen values; they keep the reference's
operation order, vectorised over layers only where numpy gives the same bits for an array as for its elements (``exp``,
``log``, ``log10`` and the four operations do; ``10 ** x`` and ``x ** 2`` do not -- a numpy scalar goes through libm's
``pow``, an array through numpy's own loop -- and stay element by element).

The grey clouds have a second form.  ``cloud_tables_batch`` turns the deck descriptions of ``S`` samples into the
``(S, 3, nlayer, nin)`` rows of their tables in ONE launch (``picaso_param_cloud_tables_dev``, csrc/paramcloud.hip) and
returns one ``ParamCloudTable`` per sample: for ``inputs.clouds(df=...)`` a dictionary like any other, for the one-call
spectrum path rows that already lie where the fused opacity launch reads them -- no host table, no digest, no upload.

Not built as methods, each refused with what is missing: the Mie clouds (``load_cld_optical`` / ``mieff_dir``,
``cloud_virga``, ``cloud_flex_fsed`` / ``flex_cloud``, ``cloud_brewster_mie``: virga; the functions of ``picaso_amd.mie``
that take a ``Parameterize`` do the last two and their batch), the Madhusudhan-Seager profiles (astropy's
``convolve``), ``chem_visscher`` (``chemeq_visscher_2121``) and ``pt_knots`` with an arbitrary ``scipy.interpolate`` name.
"""
import numpy as np

from . import justdoit as jdi

_VARS = ("opd", "w0", "g0")
_KEYS = _VARS + ("wavenumber", "pressure")
_NAN_SLAB = {"ptop": np.nan, "dp": np.nan, "reference_tau": np.nan}
_NAN_DECK = {"ptop": np.nan, "dp": np.nan}

LAUNCHES = 0            # cloud-table launches of this process so far


def _listed(x):
    """``x`` if it comes as a dictionary of ``{name: {'value': v}}``: the values in the order of the sorted names."""
    return [x[k]["value"] for k in sorted(x.keys())] if isinstance(x, dict) else x


def _missing(what, needs):
    return NotImplementedError("%s is not built here: it needs %s" % (what, needs))


class Parameterize():
    def __init__(self, load_cld_optical=None, mieff_dir=None):
        if load_cld_optical is not None or mieff_dir is not None:
            raise _missing("Parameterize(load_cld_optical=, mieff_dir=)",
                           "virga's Mie tables (virga.justdoit.get_mie), which are outside this package; "
                           "picaso_amd.mie.get_mie(gas, directory) reads a .mieff file and mie.compute_mieff makes a table here")
        self.mieff_dir = mieff_dir

    def add_class(self, picaso_inputs_class):
        """Take the pressure grid (at the very least) of a ``justdoit.inputs`` (reference parameterizations.py:40-56)."""
        self.picaso = picaso_inputs_class
        profile = picaso_inputs_class.inputs["atmosphere"]["profile"]
        self.pressure_level = np.asarray(profile["pressure"], dtype=np.float64)
        self.temperature_level = np.asarray(profile["temperature"], dtype=np.float64) \
            if "temperature" in profile.keys() else np.empty((0, 0))
        self.pressure_layer = np.sqrt(self.pressure_level[0:-1] * self.pressure_level[1:])
        self.nlevel = len(self.pressure_level)
        self.nlayer = self.nlevel - 1
        gravity = picaso_inputs_class.inputs["planet"].get("gravity", np.nan)
        self.gravity_cgs = np.nan if gravity is None else gravity      # (this package's inputs holds None until gravity())
        self.__dict__.pop("_edges", None)
        self.__dict__.pop("_resident", None)

    # ------------------------------------------------------------------------------------------ refused forms
    def cloud_virga(self, **virga_kwargs):
        raise _missing("cloud_virga", "inputs.virga and virga's Mie tables, which are outside this package (virga's cloud "
                       "model is not built; picaso_amd.mie has the size-distribution clouds, mie.cloud_flex_fsed and "
                       "mie.cloud_brewster_mie)")

    def cloud_flex_fsed(self, *args, **kwargs):
        raise _missing("cloud_flex_fsed / flex_cloud", "virga's Mie tables and calc_optics_user_r_dist, which are outside "
                       "this package; picaso_amd.mie.cloud_flex_fsed(param, table, ...) does the job here on a mie.MieTable")
    flex_cloud = cloud_flex_fsed

    def cloud_brewster_mie(self, *args, **kwargs):
        raise _missing("cloud_brewster_mie", "virga's Mie tables and calc_optics_user_r_dist, which are outside this package; "
                       "picaso_amd.mie.cloud_brewster_mie(param, table, ...) does the job here on a mie.MieTable")

    def pt_madhu_seager_09_noinversion(self, *args, **kwargs):
        raise _missing("pt_madhu_seager_09_noinversion", "astropy.convolution.convolve for its smoothing, which is not "
                       "installed with this package")

    def pt_madhu_seager_09_inversion(self, *args, **kwargs):
        raise _missing("pt_madhu_seager_09_inversion", "astropy.convolution.convolve for its smoothing, which is not "
                       "installed with this package")

    def chem_visscher(self, cto_absolute, log_mh):
        raise _missing("chem_visscher", "inputs.chemeq_visscher_2121, which this package refuses")

    # ------------------------------------------------------------------------------------------ cloud profile shapes
    def _layer_edges(self):
        """``atlev`` of every layer and the squares ``slab_decay`` takes of them, element by element as the reference
        forms them, once per pressure grid."""
        hit = self.__dict__.get("_edges")
        if hit is None or hit[0] is not self.pressure_layer:
            edges = [atlev(i, self.pressure_layer) for i in range(len(self.pressure_layer))]
            top, bot = (np.array([e[j] for e in edges]) for j in (0, 1))
            hit = self._edges = (self.pressure_layer, top, bot, np.array([t ** 2 for t in top]), np.array([b ** 2 for b in bot]))
        return hit[1:]

    def deck_decay(self, ptop, dp=0.005):
        """Optical depth per layer of a Brewster deck (reference parameterizations.py:255-286): ``ptop`` the log10 pressure
        (bar) where the cloud's optical depth reaches ~1, ``dp`` the decay scale in dex; 100 where an exponent passes 10."""
        top, bot, _, _ = self._layer_edges()
        pressure_top = 10 ** ptop
        pressure_scale = ((pressure_top * 10. ** dp) - pressure_top) / 10. ** dp
        const = 1. / (1 - np.exp(-pressure_top / pressure_scale))
        term1 = (bot - pressure_top) / pressure_scale
        term2 = (top - pressure_top) / pressure_scale
        capped = (term1 > 10) | (term2 > 10)
        with np.errstate(over="ignore", invalid="ignore"):
            opd = const * (np.exp(term1) - np.exp(term2))
        opd[capped] = 100.00
        return opd

    def slab_decay(self, ptop, dp=0.005, reference_tau=1):
        """Optical depth per layer of a Brewster slab between ``10**ptop`` and ``10**(ptop + dp)`` bar, ``reference_tau``
        in all (reference parameterizations.py:288-332; Whiteford et al., eqs. 13 and 14)."""
        pressure = self.pressure_layer
        top, bot, top_sq, bot_sq = self._layer_edges()
        opd = np.zeros(len(pressure))
        pressure_top = 10 ** ptop
        pressure_bottom = pressure_top * 10. ** dp
        logp = np.log(pressure)
        index_top = np.argmin(abs(logp - np.log(pressure_top)))
        index_bottom = np.argmin(abs(logp - np.log(pressure_bottom)))
        if index_top == index_bottom:
            raise Exception("dp entered was not large enough to create a cloud given the pressure grid spacing")
        tau_scaling = reference_tau / (pressure_bottom ** 2 - pressure_top ** 2)
        opd[index_top] = tau_scaling * (bot_sq[index_top] - pressure_top ** 2)
        opd[index_bottom] = tau_scaling * (pressure_bottom ** 2 - top_sq[index_bottom])
        inner = slice(index_top + 1, index_bottom)
        opd[inner] = tau_scaling * (bot_sq[inner] - top_sq[inner])
        return opd

    # ------------------------------------------------------------------------------------------ grey clouds
    def _grey_layers(self, decay_type, slab_kwargs, deck_kwargs):
        if decay_type == "slab":
            return self.slab_decay(**slab_kwargs)
        if decay_type == "deck":
            return self.deck_decay(**deck_kwargs)
        raise Exception("decay_type must be 'slab' or 'deck', got %r" % (decay_type,))

    def cloud_brewster_grey(self, decay_type, alpha, ssa, reference_wave=1, slab_kwargs=_NAN_SLAB, deck_kwargs=_NAN_DECK,
                            out="dataframe"):
        """Grey cloud with a slab or deck profile, single scattering albedo ``ssa``, no asymmetry and an optical depth
        that goes as ``(wavelength / reference_wave) ** -alpha`` (reference parameterizations.py:200-242), on the cloud
        wavenumber grid of ``get_cld_input_grid``.  ``out='device'`` (an addition): the same table made in HBM, a
        ``ParamCloudTable``."""
        if out == "device":
            return self.cloud_tables_batch([[dict(kind="brewster_grey", decay_type=decay_type, alpha=alpha, ssa=ssa,
                                                  reference_wave=reference_wave, slab_kwargs=slab_kwargs,
                                                  deck_kwargs=deck_kwargs)]], average=0)[0]
        import pandas as pd
        wavenumber_grid = jdi.get_cld_input_grid()
        wavelength = 1e4 / wavenumber_grid
        opd_profile = self._grey_layers(decay_type, slab_kwargs, deck_kwargs)
        opd = (opd_profile[:, None] * ((wavelength / reference_wave) ** (-alpha))[None, :]).reshape(-1)
        return pd.DataFrame({"opd": opd, "g0": opd * 0, "w0": opd * 0 + ssa,
                             "wavenumber": np.tile(wavenumber_grid, self.nlayer),
                             "pressure": np.repeat(self.pressure_layer, len(wavelength))})

    def cloud_hard_grey(self, g0, w0, opd, p, dp, out="dataframe"):
        """Box clouds through ``inputs.clouds(g0=, w0=, opd=, p=, dp=)`` of the class given to ``add_class``, which keeps
        them as its cloud profile (reference parameterizations.py:244-253).  ``out='device'`` (an addition): the table
        made in HBM, a ``ParamCloudTable``; the class is left as it is."""
        g0, w0, opd, p, dp = ([x] if isinstance(x, int) else x for x in (g0, w0, opd, p, dp))
        if out == "device":
            return self.cloud_tables_batch([[dict(kind="hard_grey", g0=g0, w0=w0, opd=opd, p=p, dp=dp)]], average=0)[0]
        import pandas as pd
        p, dp = ([float(v) for v in np.atleast_1d(x)] for x in (p, dp))       # (10 ** a negative numpy integer is an error)
        self.picaso.clouds(g0=g0, w0=w0, opd=opd, p=p, dp=dp)
        prof, grid = self.picaso.inputs["clouds"]["profile"], self.picaso.inputs["clouds"]["wavenumber"]
        cols = {"pressure": np.repeat(self.pressure_layer, len(grid)), "wavenumber": np.tile(grid, self.nlayer)}
        cols.update({k: np.asarray(prof[k], dtype=np.float64).reshape(-1) for k in ("g0", "w0", "opd")})
        return pd.DataFrame(cols)

    def _deck_record(self, deck):
        """One deck description -> ``(opd_l, w0_l, g0_l, alpha, reference_wave, parameters as floats)``: every discrete
        decision (the slab's argmin and its exception, the deck's cap, the box test) is taken here, on the host."""
        deck = dict(deck)
        kind = deck.pop("kind")
        nlayer = self.nlayer
        if kind == "brewster_grey":
            decay = deck["decay_type"]
            kw = deck.get("slab_kwargs", _NAN_SLAB) if decay == "slab" else deck.get("deck_kwargs", _NAN_DECK)
            opd_l = self._grey_layers(decay, deck.get("slab_kwargs", _NAN_SLAB), deck.get("deck_kwargs", _NAN_DECK))
            ref = deck.get("reference_wave", 1)
            par = (0.0, float(decay == "slab"), float(deck["alpha"]), float(deck["ssa"]), float(ref)) + \
                tuple(float(kw[k]) for k in sorted(kw))
            return opd_l, np.full(nlayer, float(deck["ssa"])), np.zeros(nlayer), float(deck["alpha"]), float(ref), par
        if kind == "hard_grey":
            boxes = [np.atleast_1d(np.asarray(deck[k], dtype=np.float64)) for k in ("g0", "w0", "opd", "p", "dp")]
            vec = np.zeros((3, nlayer))
            for ig, iw, io, ip, idp in zip(*boxes):                    # the box test of inputs.clouds, justdoit.py:4251-4256
                inside = (self.pressure_layer >= 10 ** (ip - idp)) & (self.pressure_layer <= 10 ** ip)
                vec[0][inside], vec[1][inside], vec[2][inside] = io, iw, ig
            par = (1.0,) + tuple(float(v) for b in boxes for v in b)
            return vec[0], vec[1], vec[2], 0.0, 1.0, par
        raise Exception("cloud_tables_batch: a deck's kind is 'brewster_grey' or 'hard_grey', got %r" % (kind,))

    def _resident_grids(self, ctx):
        """Per context: the cloud wavenumber grid and ``1e4 / wavenumber`` in HBM, with the digests the stamps carry."""
        from . import _lib
        from .device import DeviceArray
        from .optics import content_digest
        ctx = ctx if ctx is not None else _lib.context()
        grid = np.ascontiguousarray(jdi.get_cld_input_grid(), dtype=np.float64)
        key = getattr(ctx, "value", ctx)
        hit = self.__dict__.setdefault("_resident", {}).get(key)
        if hit is None or not np.array_equal(hit["grid"], grid):
            hit = self._resident[key] = dict(
                ctx=ctx, grid=grid, d_xp=DeviceArray.from_host(grid, ctx), d_wave=DeviceArray.from_host(1e4 / grid, ctx),
                device=_lib.device_of(ctx), digest=(content_digest(self.pressure_level), content_digest(grid)))
        return hit

    def _batch_records(self, decks, average=None):
        """The launch's host half: ``(layers (S, K, 3, nlayer), params (S, K, 2), average, per-sample stamps)``."""
        S = len(decks)
        K = max(len(s) for s in decks)
        if min(len(s) for s in decks) < 1 or K > 4:
            raise ValueError("cloud_tables_batch: every sample takes 1 to 4 decks")
        average = int(K > 1) if average is None else int(bool(average))
        if not average and K != 1:
            raise ValueError("cloud_tables_batch: average=0 takes one deck per sample")
        layers, params = np.zeros((S, K, 3, self.nlayer)), np.zeros((S, K, 2))
        params[:, :, 1] = 1.0
        stamps = []
        for s, sample in enumerate(decks):
            pars = []
            for k, deck in enumerate(sample):
                layers[s, k, 0], layers[s, k, 1], layers[s, k, 2], params[s, k, 0], params[s, k, 1], par = self._deck_record(deck)
                pars.append(par)
            stamps.append(tuple(pars))
        return layers, params, average, stamps

    def cloud_tables_batch(self, decks, average=None, ctx=None):
        """The cloud tables of ``S`` samples in ONE launch.  ``decks``: a list of ``S`` samples, each a list of 1 to 4 deck
        descriptions -- the keyword dictionary of ``cloud_brewster_grey`` or of ``cloud_hard_grey`` with a ``kind`` key
        (``'brewster_grey'`` / ``'hard_grey'``).  ``average``: 1 combines every sample's decks with the arithmetic of
        ``cloud_averaging`` (a sample of one deck goes through it too, as ``cloud_averaging([df])`` would), 0 stores the
        one deck of every sample as it is; default 1 when a sample has more than one deck.  A sample with fewer decks than
        the longest is filled up with empty ones, which add ``+0`` to every sum.  Returns ``S`` ``ParamCloudTable``, all
        views of one ``(S, 3, nlayer, nin)`` device array."""
        global LAUNCHES
        from . import _lib, device
        from .device import DeviceArray
        S = len(decks)
        if S == 0:
            return []
        layers, params, average, stamps = self._batch_records(decks, average)
        K, nlayer = layers.shape[1], self.nlayer
        with _lib.CALL_LOCK:
            res = self._resident_grids(ctx)
            ctx, nin = res["ctx"], res["grid"].size
            d_layers, d_params = DeviceArray.from_host(layers, ctx), DeviceArray.from_host(params, ctx)
            out = DeviceArray((S, 3 * nlayer, nin), ctx)
            _lib.check(_lib.load().picaso_param_cloud_tables_dev(ctx, S, K, nlayer, nin, average, d_layers.addr, d_params.addr,
                                                                 res["d_wave"].addr, out.addr), ctx)
            LAUNCHES += 1
            # read from other contexts' streams of this device (an opacity object's): written before anyone can ask for
            # them.  One wait per batch; it also covers the record uploads going out of scope
            device.sync(ctx)
        return [ParamCloudTable(res, self.pressure_layer, out.row_block(s), nlayer, res["digest"] + (average, stamps[s]))
                for s in range(S)]

    # ------------------------------------------------------------------------------------------ chemistry
    def chem_free(self, **species):
        """Abundance per level for free chemistry (reference parameterizations.py:334-381): every species a dictionary with
        a well-mixed ``value`` or a ``profile`` (``'knots'`` / ``'gradient'``, the ``vmr_*`` below); ``background`` =
        ``dict(gases=[one])`` takes what is left of 1, ``dict(gases=[a, b], fraction=a/b)`` shares it."""
        import pandas as pd
        pressure_grid, temp_grid = self.pressure_level, self.temperature_level
        total = 0 * pressure_grid
        assert len(temp_grid) == len(pressure_grid), \
            "Len of t grid does not match len of p grid. likely t grid has not been set yet "
        df = pd.DataFrame(dict(pressure=pressure_grid, temperature=temp_grid))
        for name in species.keys():
            if name == "background":
                continue
            value = species[name].get("value", None)
            if value is not None:
                df[name] = value
            else:
                df[name] = getattr(self, "vmr_%s" % species[name]["profile"])(species[name])
            total += df[name].values
        if "background" in species.keys():
            rest = 1 - total
            gases = species["background"]["gases"]
            if len(gases) == 2:
                fraction = species["background"]["fraction"]
                second = rest / (fraction + 1)
                df[gases[0]] = fraction * second
                df[gases[1]] = second
            if len(gases) == 1:
                df[gases[0]] = rest
        return df

    def vmr_knots(self, species):
        """log-log linear interpolation (and extrapolation) of ``vmr_knots`` at ``P_knots`` (reference :383-393)."""
        from scipy import interpolate
        abun_knots = _listed(species["vmr_knots"])
        P_knots = _listed(species["P_knots"])
        f = interpolate.interp1d(np.log10(P_knots), np.log10(abun_knots), kind="linear", bounds_error=False,
                                 fill_value="extrapolate")
        return 10 ** f(np.log10(self.pressure_level))

    def vmr_gradient(self, species):
        """Constant ``bottom`` (or ``top``) value with a power law of slope ``gradient`` in log10 P on the other side of
        ``p_switch``, capped at 1 (reference :395-436)."""
        deep = species.get("bottom", None)
        n = 1 if deep is None else 0
        ct = species["top"]["value"] if deep is None else deep["value"]
        p_switch, gradient = species["p_switch"]["value"], species["gradient"]["value"]
        vmr = ct + 0 * self.pressure_level
        sign = (-1) ** n
        for i, p in enumerate(self.pressure_level):         # (10 ** x of a numpy scalar is libm's pow: element by element)
            if sign * p <= sign * p_switch:
                vmr[i] = 10 ** (np.log10(ct) + (gradient * (abs(np.log10(p) - np.log10(p_switch)))))
        vmr[vmr > 1] = 1
        return vmr

    # ------------------------------------------------------------------------------------------ T(P)
    def pt_knots(self, P_knots, T_knots, interpolation="brewster", scipy_interpolate_kwargs={}):
        """Temperature at ``P_knots`` (any order; lists or ``{name: {'value': v}}``) interpolated in log10 P (reference
        :520-570): ``'brewster'`` (the absolute value of an interpolating cubic B-spline, 4 knots), ``'linear'`` (2),
        ``'quadratic_spline'`` (3) or ``'cubic_spline'`` (4)."""
        import pandas as pd
        from scipy import interpolate
        P_knots, T_knots = _listed(P_knots), _listed(T_knots)
        pressure = self.pressure_level
        order = np.argsort(P_knots)
        P_knots, T_knots = np.array(P_knots)[order], np.array(T_knots)[order]
        kinds = {"linear": ("linear", 2), "quadratic_spline": ("quadratic", 3), "cubic_spline": ("cubic", 4)}
        if interpolation == "brewster":
            spline = interpolate.splrep(np.log10(P_knots), T_knots, s=0)
            temp = np.abs(interpolate.splev(np.log10(pressure), spline, der=0))
        elif interpolation in kinds:
            kind, least = kinds[interpolation]
            assert len(P_knots) >= least, "%s splines require at least %d knots" % (kind.capitalize(), least)
            f = interpolate.interp1d(np.log10(P_knots), T_knots, kind=kind, bounds_error=False, fill_value="extrapolate")
            temp = f(np.log10(pressure))
        elif hasattr(interpolate, str(interpolation)):
            raise _missing("pt_knots(interpolation=%r)" % (interpolation,), "a call convention for arbitrary scipy.interpolate "
                           "objects; 'brewster', 'linear', 'quadratic_spline' and 'cubic_spline' are built")
        else:
            raise Exception("Unknown interpolation method '%s'" % (interpolation,))
        return pd.DataFrame(dict(pressure=pressure, temperature=temp))

    def pt_zj24(self, pressures, dTs, Tbottom):
        """Zhang et al. 2024: d ln T / d ln P at ``pressures`` (quadratic in ln P), integrated upwards from
        ``Tbottom['value']`` at the deepest level (reference :572-595)."""
        import pandas as pd
        from scipy import interpolate
        pressures, dTs = _listed(pressures), _listed(dTs)
        pressure = self.pressure_level
        T = np.zeros(len(pressure))
        log_rev = np.log(pressure[::-1])
        f = interpolate.interp1d(np.log(pressures), dTs, kind="quadratic", bounds_error=False, fill_value="extrapolate")
        grad = f(log_rev)
        T[0] = Tbottom["value"]
        for i in range(1, len(pressure)):
            T[i] = np.exp(np.log(T[i - 1]) + (log_rev[i] - log_rev[i - 1]) * grad[i - 1])
        return pd.DataFrame(dict(pressure=pressure, temperature=T[::-1]))

    def pt_guillot(self, Teq, T_int, logg1, logKir, alpha):
        """Guillot (2010) profile with two equal visible channels, ``kv = 10**(logg1 + logKir)``, ``kth = 10**logKir``,
        on 300 optical depths and interpolated to the pressure levels in log10 P (reference :597-656)."""
        import pandas as pd
        from scipy import special
        kv1, kv2 = 10. ** (logg1 + logKir), 10. ** (logg1 + logKir)
        kth = 10. ** logKir
        f = 1.0
        g0 = self.gravity_cgs / 100.0
        assert not np.isnan(g0), "Graivty was not supplied but is being requested for guillot p-t profile parameterization"
        tau = 10 ** np.arange(-10, 20, .1)
        T4ir = 0.75 * (T_int ** (4.)) * (tau + (2.0 / 3.0))

        def channel(gamma):
            return (2.0 / 3.0 + 2.0 / (3.0 * gamma) * (1. + (gamma * tau / 2.0 - 1.0) * np.exp(-gamma * tau))
                    + 2.0 * gamma / 3.0 * (1.0 - tau ** 2.0 / 2.0) * special.expn(2.0, gamma * tau))
        T4v1 = f * 0.75 * Teq ** 4.0 * (1.0 - alpha) * channel(kv1 / kth)
        T4v2 = f * 0.75 * Teq ** 4.0 * alpha * channel(kv2 / kth)
        T = (T4ir + T4v1 + T4v2) ** (0.25)
        P = tau * g0 / (kth * 0.1) / 1.E5
        T = np.interp(np.log10(self.pressure_level), np.log10(P), T)
        return pd.DataFrame({"temperature": T, "pressure": self.pressure_level})

    def pt_isothermal(self, T):
        import pandas as pd
        return pd.DataFrame({"temperature": T, "pressure": self.pressure_level})


def atlev(l0, pressure_layer):
    """Top and bottom pressure of layer ``l0`` from the layer pressures, half-way in log P to its neighbours (reference
    parameterizations.py:661-670)."""
    p = pressure_layer
    if l0 <= p.size - 2:
        top = np.exp(1.5 * np.log(p[l0]) - 0.5 * np.log(p[l0 + 1]))
        bottom = np.exp(0.5 * np.log(p[l0] * p[l0 + 1]))
    else:                                   # the last layer: mirrored about its own pressure
        top = np.exp(0.5 * np.log(p[l0 - 1] * p[l0]))
        bottom = p[l0] ** 2 / top
    return top, bottom


def picaso_format(opd, w0, g0, wavenumber_grid, pressure_grid, p_bottom=None, p_top=None, p_decay=None, opd_profile=None):
    """A wavelength-dependent aerosol (``opd``, ``w0``, ``g0`` on ``wavenumber_grid``) laid on the layers between
    ``p_top`` and ``p_bottom`` (bar) as a cloud DataFrame, zero elsewhere: as it is, times ``p_decay / max(p_decay)``, or
    as ``opd_profile`` times ``opd / max(opd)`` (reference parameterizations.py:672-750)."""
    import pandas as pd
    if p_bottom is None:
        p_bottom = np.max(pressure_grid) + 10
    if p_top is None and p_decay is None and opd_profile is None:
        raise Exception("Must specify cloud top pressure via p_top, or the vertical pressure decay via p_decay, or an opd "
                        "profile via opd_profile")
    if p_top is None:
        p_top = 1e-10
    opd, w0, g0 = (np.asarray(x, dtype=np.float64) for x in (opd, w0, g0))
    pressure_grid = np.asarray(pressure_grid, dtype=np.float64)
    nlay, nw = pressure_grid.shape[0], opd.shape[0]
    inside = ((p_top <= pressure_grid) & (pressure_grid <= p_bottom))[:, None]
    if p_decay is None and opd_profile is None:
        scaled = np.broadcast_to(opd, (nlay, nw))
    elif p_decay is not None:
        scaled = (np.asarray(p_decay, dtype=np.float64) / np.max(p_decay))[:, None] * opd[None, :]
    else:
        scaled = np.asarray(opd_profile, dtype=np.float64)[:, None] * (opd / np.max(opd))[None, :]
    cols = {"pressure": np.repeat(pressure_grid, nw), "wavenumber": np.tile(np.asarray(wavenumber_grid)[:nw], nlay)}
    for name, full, one in (("opd", scaled, opd), ("w0", w0[None, :], w0), ("g0", g0[None, :], g0)):
        cols[name] = np.where(inside, full, one[None, :] * 0).reshape(-1)
    return pd.DataFrame(cols, columns=["pressure", "wavenumber", "opd", "w0", "g0"])


def cloud_averaging(dfs):
    """One cloud table from a list of tables on the same grid (reference parameterizations.py:753-792): the optical depths
    add, ``w0`` and ``g0`` are their optical-depth-weighted means, and a zero optical depth becomes 1e-33.  As in the
    reference the result is ``dfs[0]`` itself with the three columns replaced."""
    tables = [(df["opd"].values, df["g0"].values, df["w0"].values) for df in dfs]
    opd, g0, w0 = (0 * tables[0][0] for _ in range(3))
    for t_opd, _, _ in tables:
        assert len(opd) == len(t_opd), "cloud dataframes were made on different grids"
        opd += t_opd
    for t_opd, t_g0, t_w0 in tables:
        g0 += t_opd * t_g0
        w0 += t_opd * t_w0
    opd[opd == 0] = 1e-33                   # before the quotients, as the reference does
    out = dfs[0]
    out["opd"], out["g0"], out["w0"] = opd, g0 / opd, w0 / opd
    return out


class ParamCloudTable(dict):
    """The cloud table of one sample, made in HBM by ``Parameterize.cloud_tables_batch``: what ``inputs.clouds(df=...)``
    may be given in place of a DataFrame.  Two faces, as ``gcm.FacetCloudTables``:

    * resident: ``d_xp`` (the wavenumber grid), ``d_stack`` (the ``(3 * nlayer, nin)`` rows opd, w0, g0 where they lie)
      and ``stamp`` (the digests of the pressure and the wavenumber grid, the averaging flag and the deck parameters as
      floats: an identity of the table's content for a caller's own memo.  Nothing in the package compares it yet: the
      rows are read where they lie, so there is no device copy to key).  ``resident_tables(nlayer, ctx)`` hands them out as ``(nin, d_xp, d_stack, stamp)`` for a
      context on the table's device, else ``None``: the caller goes on with the dictionary face.
    * a dictionary: ``opd``, ``w0``, ``g0``, ``pressure`` and ``wavenumber`` appear on first use, by one copy back, as the
      ``nlayer * nin`` columns of the DataFrame ``cloud_brewster_grey`` returns (layer by layer, wavenumber increasing).
      ``materialized`` says whether that has happened.

    The object is not meant to be edited; a deep copy is the object itself, a pickle is the plain host dictionary."""

    def __init__(self, resident, pressure_layer, d_stack, nlayer, stamp):
        dict.__init__(self)
        self.resident, self.d_xp, self.d_stack, self.stamp = resident, resident["d_xp"], d_stack, stamp
        self.grid, self.pressure_layer = resident["grid"], pressure_layer
        self.nlayer, self.nin = int(nlayer), int(self.grid.size)
        self.materialized = False

    # ---- the resident face
    def resident_tables(self, nlayer, ctx):
        from . import _lib
        if nlayer != self.nlayer or self.nin < 2:
            return None
        own = self.resident["ctx"]
        if getattr(ctx, "value", ctx) != getattr(own, "value", own) and _lib.device_of(ctx) != self.resident["device"]:
            return None
        return self.nin, self.d_xp, self.d_stack, self.stamp

    # ---- the dictionary face
    def _rows(self):
        """The ``(3, nlayer, nin)`` rows on the host (the one copy back)."""
        return self.d_stack.to_host().reshape(3, self.nlayer, self.nin)

    def _fill(self):
        if self.materialized:
            return
        for k, a in zip(_VARS, self._rows()):
            dict.__setitem__(self, k, a.reshape(-1))
        dict.__setitem__(self, "wavenumber", np.tile(self.grid, self.nlayer))
        dict.__setitem__(self, "pressure", np.repeat(self.pressure_layer, self.nin))
        self.materialized = True

    def __getitem__(self, key):
        self._fill()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        self._fill()
        return dict.get(self, key, default)

    def __contains__(self, key):
        return key in _KEYS

    def __len__(self):
        return len(_KEYS)

    def __iter__(self):
        self._fill()
        return dict.__iter__(self)

    def keys(self):
        self._fill()
        return dict.keys(self)

    def items(self):
        self._fill()
        return dict.items(self)

    def values(self):
        self._fill()
        return dict.values(self)

    def copy(self):
        return dict(self.items())

    def _frozen(self, *args, **kwargs):
        raise TypeError("a ParamCloudTable is not editable: take dict(table) and edit that")

    __setitem__ = __delitem__ = update = pop = popitem = clear = setdefault = _frozen

    def __deepcopy__(self, memo):
        return self

    __copy__ = lambda self: self

    def __reduce__(self):
        return dict, (dict(self.items()),)
