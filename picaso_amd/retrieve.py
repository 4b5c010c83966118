"""Configuration and parameter cube -> batched log-likelihoods: the reference's retrieval driver (picaso/driver.py) on the
batched paths of this package.

The reference's ``MODEL`` runs one proposal at a time: it writes the row into the configuration, builds an ``inputs``
object, runs ``spectrum()`` and bins the full-resolution result on the host once per data set (driver.py:214-236).  Here a
``(N, ndim)`` cube builds the ``N`` objects and then takes ONE launch per stage:

* ``chemistry.method = 'visscher'``: one ``chemistry.chem_interp_batch`` call per grid file (``cto_absolute`` / ``log_mh`` may
  be fitted, so samples are grouped by ``select_visscher_2121``'s file), ``(n, nlevel)`` points each;
* clouds: one ``Parameterize.cloud_tables_batch`` call when every deck of the batch is grey, one
  ``mie.cloud_tables_batch`` call when every deck is a Mie deck; anything else takes the host functions per sample;
* spectra: ``spectrum_batch(cases, OPA, instruments=plan)``: every data set, binned (``mean_regrid``) or convolved
  (``conv_non_uniform_R``), comes from ONE ``picaso_instruments_reduce_dev`` call per spectrum (csrc/instruments.hip), with
  the reference's flux scale ``1e-8 (R / d)^2`` applied per column before the sums, as the reference applies it before it
  bins.

A row goes the same way whatever batch it comes in (``N = 1`` included), so its result does not depend on ``N``.  The
likelihood stays host numpy in the reference's operation order: given the same binned model it is the reference's number.

This is host Python; ``picaso_amd/driver.py`` is the C spectrum driver and keeps its name.  Not here: a sampler, an MPI
pool, ``retrieve()`` and the ``viz`` / plot functions.  ``pt_`` / ``chem_`` / ``cloud_`` kinds that ``Parameterize`` refuses
(virga, Madhusudhan-Seager, and ``sonora_bobcat`` through ``inputs.sonora``) keep refusing with their own messages.
"""
import os
from collections.abc import Mapping
from functools import partial

import numpy as np

from . import chemistry
from . import justdoit as jdi
from . import regrid as _regrid
from .parameterizations import Parameterize, cloud_averaging

chem_options = ['visscher', 'free', 'userfile']
cloud_options = ['brewster_grey', 'brewster_mie', 'virga', 'flex_fsed', 'hard_grey', 'userfile']
pt_options = ['userfile', 'isothermal', 'knots', 'guillot', 'sonora_bobcat', 'madhu_seager_09_inversion',
              'madhu_seager_09_noinversion', 'zj_24']

_GREY = ("brewster_grey", "hard_grey")
_MIE = ("brewster_mie", "flex_fsed")
_NOT_MODEL = ("offset", "scaling", "err_inf")          # cube entries the likelihood reads, not the model


# ---------------------------------------------------------------------------------------------------------------------
# dictionaries and priors
# ---------------------------------------------------------------------------------------------------------------------
def prior_finder(d):
    """Every section of ``d`` that holds a ``prior`` key, as ``{dotted.path: section}``: a depth-first walk that names a
    section before the sections below it and keeps the dictionaries' own order (reference driver.py:143-156)."""
    sections = {}
    todo = [((), d)] if isinstance(d, Mapping) else []
    while todo:
        path, node = todo.pop()
        if "prior" in node:
            sections[".".join(path)] = node
        below = [(path + (name,), child) for name, child in node.items() if isinstance(child, Mapping)]
        todo.extend(reversed(below))
    return sections


def set_dict_value(data, path_string, new_value):
    """Replace the value at the dot-separated ``path_string`` of the nested dictionary ``data``.  Only a key that is
    already there is written: True then; otherwise a printed note and False, and ``data`` is as it was (reference
    driver.py:640-675)."""
    *parents, last = path_string.split(".")
    node = data
    for name in parents:
        node = node.get(name) if isinstance(node, dict) else None
        if not isinstance(node, dict):
            print("set_dict_value: no dictionary at %r on the way to %r" % (name, path_string))
            return False
    if last not in node:
        print("set_dict_value: %r names no existing key" % (path_string,))
        return False
    node[last] = new_value
    return True


def find_values_for_key(data, target_key):
    """The values stored under ``target_key`` anywhere in ``data``, through nested dictionaries and dictionaries inside
    lists, as strings (reference driver.py:678-711).  As there, a hit folds everything found so far in that dictionary,
    the hit included (a string as one value, a list as its members), into its sorted distinct strings; what is found below
    later keys is appended as it comes."""
    if not isinstance(data, dict):
        return []
    found = []
    for key, value in data.items():
        if key == target_key:
            found = [str(v) for v in np.unique(found + [[value] if isinstance(value, str) else value])]
            continue
        children = [value] if isinstance(value, dict) else value if isinstance(value, list) else []
        for child in children:
            found += find_values_for_key(child, target_key)
    return found


def _unit_to_prior(section, u):
    """One parameter's prior transform of ``u`` (a scalar or a column), before ``log``."""
    kind = section['prior']
    if kind == 'uniform':
        lo, hi = section['uniform_kwargs']['min'], section['uniform_kwargs']['max']
        return lo + (hi - lo) * u
    if kind == 'gaussian':
        from scipy import stats
        return stats.norm.ppf(u, loc=section['gaussian_kwargs']['mean'], scale=section['gaussian_kwargs']['std'])
    raise Exception('Prior type not available')


def hypercube(u, fitpars):
    """Unit cube -> parameters (reference driver.py:158-174): ``uniform`` is ``min + (max - min) u``, ``gaussian``
    ``scipy.stats.norm.ppf``, and ``log`` takes ``10 ** x`` of the result.  ``u`` of shape ``(ndim,)`` as the reference;
    ``(N, ndim)`` in addition, every row with the bits of its own call: the sums, products and ``ppf`` are the same element
    by element for an array, ``10 ** x`` is not (an array goes through numpy's loop, a scalar through libm's ``pow``) and is
    taken scalar by scalar."""
    u = np.asarray(u)
    if u.ndim not in (1, 2):
        raise Exception("hypercube: u has shape %s; (ndim,) or (N, ndim)" % (u.shape,))
    columns = u.T                                       # one entry per parameter: a scalar, or the N values of a batch
    x = np.empty(columns.shape)
    for i, section in enumerate(fitpars.values()):
        x[i] = _unit_to_prior(section, columns[i])
        if section['log']:
            x[i] = [10 ** v for v in x[i]] if u.ndim == 2 else 10 ** x[i]
    return x.T


# ---------------------------------------------------------------------------------------------------------------------
# configuration -> inputs
# ---------------------------------------------------------------------------------------------------------------------
def pressure_grid(P_config):
    """The level pressures (bar) of ``P_config = dict(min={value, unit}, max={value, unit}, nlevel=n, spacing='log' |
    'linear')``: ``np.logspace(log10 min, log10 max, n)`` or ``np.linspace`` (reference justdoit.py:3249-3281).  Units: the
    pressure names of ``justdoit`` (bar, mbar, Pa, atm, ...)."""
    def bar(which):
        entry = P_config.get(which, {})
        value, unit = entry.get('value'), entry.get('unit')
        if value is None:
            raise Exception("pressure_grid: P_config[%r] needs a value (and a unit; bar when none is given)" % which)
        fac = jdi._PRESSURE_TO_BAR.get(str('bar' if unit is None else unit).strip().lower())
        if fac is None:
            raise Exception("pressure_grid: pressure unit %r not known; one of %s" % (unit, sorted(jdi._PRESSURE_TO_BAR)))
        return value * fac
    minp_bar, maxp_bar = bar('min'), bar('max')
    nlevel = P_config.get('nlevel')
    if P_config.get('spacing') == 'log':
        return np.logspace(np.log10(minp_bar), np.log10(maxp_bar), nlevel)
    return np.linspace(minp_bar, maxp_bar, nlevel)


def _quantity(section, name, what):
    """``section[name] = {value, unit}`` in cgs (radians for an angle), None when there is no value."""
    entry = section.get(name, {}) or {}
    value = entry.get('value', None)
    return None if value is None else jdi._to_cgs(value, entry.get('unit', None), what)


def PT_handler(pt_config, picaso_class, param_tools):
    """The T(P) table of ``pt_config`` (reference driver.py:610-637): a ``userfile``, or the pressure grid of
    ``pt_config['pressure']`` with ``param_tools.pt_<profile>(**pt_config[<profile>])``."""
    kind = pt_config['profile']
    if kind == 'userfile':
        import pandas as pd
        return pd.read_csv(pt_config['userfile']['filename'], **pt_config['userfile'].get('pd_kwargs', {}))
    if kind == 'sonora_bobcat':
        picaso_class.sonora(**pt_config.get('sonora_bobcat', {}))
        return picaso_class.inputs['atmosphere']['profile']
    picaso_class.add_pt(P=pressure_grid(pt_config['pressure']))          # (the reference's add_pt(P_config=))
    param_tools.add_class(picaso_class)
    return getattr(param_tools, f'pt_{kind}')(**pt_config[kind])


_files = {}            # path -> ((mtime_ns, size), what was read): the grid and .mieff files a retrieval reads per proposal


def _read_once(path, read):
    """``read(path)``, kept per process until the file changes (16 files, then the memo starts again, as the plan memos)."""
    st = os.stat(path)
    stamp = (st.st_mtime_ns, st.st_size)
    hit = _files.get(path)
    if hit is None or hit[0] != stamp:
        if len(_files) > 16:
            _files.clear()
        hit = _files[path] = (stamp, read(path))
    return hit[1]


def _chem_visscher(cases, params):
    """``chemeq_visscher_2121(cto_absolute, log_mh)`` for every case: the species of the nearest grid file join its profile.
    One ``chemistry.chem_interp_batch`` launch per file for all the cases that select it; a case alone takes the same
    launch, so its abundances do not depend on its company."""
    def value(x):                                    # a fitted entry is {'value': v}: MODEL writes the row's value there
        return x['value'] if isinstance(x, Mapping) else x
    groups = {}
    for j, kw in enumerate(params):
        filename = chemistry.select_visscher_2121(value(kw['cto_absolute']), value(kw['log_mh']))
        groups.setdefault(filename, []).append(j)
    for filename, members in groups.items():
        profs = [cases[j].inputs['atmosphere']['profile'] for j in members]
        t = np.array([np.asarray(p['temperature'], dtype=float) for p in profs])
        p = np.array([np.asarray(p['pressure'], dtype=float) for p in profs])
        out = chemistry.chem_interp_batch(t, p, _read_once(filename, chemistry.read_visscher_2121))
        for i, j in enumerate(members):
            df = {k: np.asarray(profs[i][k]) for k in profs[i].keys()}           # chem_interp adds to the profile
            df.update({k: np.ascontiguousarray(v[i]) for k, v in out.items()})
            cases[j].atmosphere(df=df)


def _mie_table(kwargs, config):
    """The ``mie.MieTable`` of a Mie deck: ``table`` of its keywords, or the ``.mieff`` file of its ``condensate`` under
    ``config['OpticalProperties']['virga_mieff']`` (``mie.get_mie``'s file, read once: ``_read_once``)."""
    from . import mie
    table = kwargs.get('table')
    if table is not None:
        return table
    directory = config.get('OpticalProperties', {}).get('virga_mieff', None)
    gas = kwargs.get('condensate')
    if gas is None or directory is None:
        raise Exception("a brewster_mie / flex_fsed cloud needs table = a mie.MieTable, or a condensate and "
                        "OpticalProperties.virga_mieff = the directory of its .mieff file")
    return _read_once(os.path.join(str(directory), "%s.mieff" % gas), mie.read_mieff)


def _cloud_decks(config):
    """``[(kind, keywords)]`` of the configuration's clouds in its order, None without a ``clouds`` section (the reference's
    ``<name>_type`` entries, driver.py:583-601)."""
    cloud_config = config.get('clouds', None)
    if not isinstance(cloud_config, dict):
        return None
    names = [i.split('_type')[0] for i in cloud_config.keys() if 'type' in i]
    return [(cloud_config[f'{n}_type'], cloud_config[n][cloud_config[f'{n}_type']]) for n in names]


def _deck_record(kind, kwargs, config):
    """The deck description the batched cloud calls take."""
    deck = {k: v for k, v in kwargs.items() if k not in ('condensate', 'table')}
    deck['kind'] = kind
    if kind in _MIE:
        deck['table'] = _mie_table(kwargs, config)
    return deck


def _cloud_host(kind, kwargs, config, param_tools):
    """One deck through the host functions: the reference's ``cloud_<kind>(**kwargs)`` or its ``userfile``."""
    if kind == 'userfile':
        import pandas as pd
        return pd.read_csv(kwargs['filename'], **kwargs.get('pd_kwargs', {}))
    if kind in _MIE:
        from . import mie
        rest = {k: v for k, v in kwargs.items() if k not in ('condensate', 'table')}
        return getattr(mie, f'cloud_{kind}')(param_tools, _mie_table(kwargs, config), **rest)
    return getattr(param_tools, f'cloud_{kind}')(**kwargs)


def _setup_base(config, opacity, param_tools):
    """``setup_spectrum_class`` up to the chemistry (reference driver.py:494-563) and the chemistry itself unless it is
    ``visscher``, which the caller batches.  Returns ``(inputs, visscher keywords or None)``."""
    def entry(section, name):
        """``(value, unit)`` of ``section[name]``; Nones where the configuration has no such entry."""
        e = section.get(name) or {}
        return e.get('value'), e.get('unit')
    irradiated = config['irradiated']
    A = jdi.inputs(calculation='planet' if irradiated else 'browndwarf', climate=False)
    rad = _quantity(config.get('geometry', {}), 'phase', 'angle')
    A.phase_angle(0 if rad is None else rad)
    (g, g_unit), (r, r_unit), (m, m_unit) = (entry(config['object'], k) for k in ('gravity', 'radius', 'mass'))
    if g is not None:                                    # gravity (and the radius beside it) first, else radius and mass
        A.gravity(gravity=g, gravity_unit=g_unit, radius=r, radius_unit=r_unit)
    else:
        A.gravity(radius=r, radius_unit=r_unit, mass=m, mass_unit=m_unit)
    if irradiated:
        star = config['star']
        spectrum = dict(filename=None, w_unit=None, f_unit=None)
        model = dict(temp=None, metal=None, logg=None, database="ck04models")
        if star.get('type') == 'userfile':
            spectrum.update({k: star.get('userfile', {}).get(k) for k in spectrum})
            if not os.path.exists(str(spectrum['filename'])):
                raise Exception("star.userfile.filename %r does not exist" % (spectrum['filename'],))
        else:
            grid = star.get('grid', {})
            model.update(temp=grid.get('teff'), metal=grid.get('feh'), logg=grid.get('logg'),
                         database=grid.get('database', model['database']))
        (rs, rs_unit), (sa, sa_unit) = entry(star, 'radius'), entry(star, 'semi_major')
        A.star(opacity, radius=rs, radius_unit=rs_unit, semi_major=sa, semi_major_unit=sa_unit, **model, **spectrum)
    A.atmosphere(df=PT_handler(config['temperature'], A, param_tools))      # includes chemistry if the userfile has it
    param_tools.add_class(A)
    chem_config = config.get('chemistry', {})
    chem_type = chem_config.get('method', '')
    if chem_type == 'visscher':
        return A, chem_config[chem_type]
    if chem_type == 'userfile':
        import pandas as pd
        table = pd.read_csv(chem_config[chem_type]['filename'], **chem_config[chem_type].get('pd_kwargs', {}))
        prof = A.inputs['atmosphere']['profile']
        n = min(len(table), len(prof['pressure']))       # level by level; the file's own T and P give way to the profile's
        df = {k: np.asarray(prof[k])[:n] for k in ('temperature', 'pressure')}
        df.update({k: table[k].values[:n] for k in table.columns if k not in df})
        A.atmosphere(df=df)
    elif chem_type != '':
        A.atmosphere(df=getattr(param_tools, f'chem_{chem_type}')(**chem_config[chem_type]))
    else:
        A.atmosphere()                                   # (the reference's df_mixingratio is unbound here)
    return A, None


def setup_spectrum_class(config, opacity, param_tools):
    """The ``inputs`` object of a configuration (reference driver.py:484-607): browndwarf or planet, ``phase_angle``,
    ``gravity`` (gravity + radius, else radius + mass), ``star`` when ``irradiated``, T(P), chemistry (``free``,
    ``visscher``, ``userfile``), clouds (every ``<name>_type``, ``cloud_averaging`` over them, ``clouds(df=)``).  Units are
    the strings of ``justdoit`` (or astropy units, where astropy is installed).  The clouds go through the host functions;
    ``MODEL`` makes the same tables on the device, a batch at a time."""
    if opacity is None:
        op = config['OpticalProperties']
        opacity = jdi.opannection(filename_db=op['opacity_files'], method=op['opacity_method'], **op.get('opacity_kwargs', {}))
    A, visscher = _setup_base(config, opacity, param_tools)
    if visscher is not None:
        _chem_visscher([A], [visscher])
    decks = _cloud_decks(config)
    if decks is not None:
        A.clouds(df=cloud_averaging([_cloud_host(kind, kw, config, param_tools) for kind, kw in decks]))
    return A


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def get_data(config):
    """``{name: [wavenumber ascending, y, e]}`` (and ``R`` as a fourth entry where the data set has one) for EVERY entry of
    ``config['InputOutput']['observation_data']`` (reference driver.py:81-141, whose loop overwrites its result and returns
    the last one only).  An entry is a dictionary of arrays ``{wavelength [um], y, e}`` with an optional ``R``, a text file of
    3 or 4 such columns (``np.loadtxt``), or a ``.nc`` file as the reference reads it (needs xarray)."""
    obs_type = config['observation_type']
    to_fit = 'transit_depth' if obs_type == 'transmission' else 'flux'
    returns = {}
    for key, obs in config['InputOutput']['observation_data'].items():
        R = None
        if isinstance(obs, Mapping):
            wl, y, e = (np.asarray(obs[k], dtype=float) for k in ('wavelength', 'y', 'e'))
            R = obs.get('R', None)
        elif str(obs).endswith('.nc'):
            try:
                import xarray as xr
            except ImportError:
                raise ImportError("get_data: %r is a netCDF file, which is read with xarray, and xarray is not installed; "
                                  "give the data as arrays {wavelength, y, e} or as a text file of 3 or 4 columns" % (obs,))
            dat = xr.load_dataset(obs)
            wl = np.asarray(dat.coords['wavelength'].values, dtype=float)
            y = np.asarray(dat.data_vars[to_fit].values, dtype=float)
            e = np.asarray(dat.data_vars[to_fit + '_error'].values, dtype=float)
        else:
            cols = np.loadtxt(obs, ndmin=2)
            if cols.shape[1] not in (3, 4):
                raise Exception("get_data: %r has %d columns; wavelength [um], y, e and optionally R" % (obs, cols.shape[1]))
            wl, y, e = cols[:, 0], cols[:, 1], cols[:, 2]
            R = cols[:, 3] if cols.shape[1] == 4 else None
        wavenumber = 1e4 / wl
        order = np.argsort(wavenumber, kind='stable')
        returns[key] = [wavenumber[order], y[order], e[order]]
        if R is not None:
            R = np.asarray(R, dtype=float)
            returns[key].append(R[order] if R.ndim == 1 else np.full(wl.shape, float(R)))
    return returns


def _instruments(config, DATA_DICT):
    """The ``instruments=`` dictionary of the data: a set with ``R`` is convolved with ``conv_non_uniform_R``'s Gaussian at
    its wavelengths, one without is binned by ``mean_regrid(newx=wavenumber)``."""
    spec = {}
    for key in config['InputOutput']['observation_data']:
        data = DATA_DICT[key]
        spec[key] = {'newx': data[0]} if len(data) < 4 else {'wl': 1e4 / data[0], 'R': data[3]}
    return spec


# ---------------------------------------------------------------------------------------------------------------------
# the model and the likelihood
# ---------------------------------------------------------------------------------------------------------------------
def _copy_config(d):
    """The dictionaries and lists of ``d`` copied, the leaves shared: ``MODEL`` writes every row into its own copy."""
    if isinstance(d, dict):
        return {k: _copy_config(v) for k, v in d.items()}
    if isinstance(d, list):
        return [_copy_config(v) for v in d]
    return d


def _flux_scale(config):
    """``1e-8 (R / d)^2`` of reference driver.py:224-230."""
    R = _quantity(config['object'], 'radius', 'radius')
    d = _quantity(config['object'], 'distance', 'distance')
    if R is None or d is None:
        raise Exception("MODEL: a thermal model is 1e-8 (R / d)^2 out['thermal'] and needs object.radius and object.distance")
    return 1e-8 * (R / d) ** 2


def _batch_clouds(cases, decks, configs, param_tools):
    """The cloud tables of the batch: ONE launch when every deck is grey, or every deck is a Mie deck, and all cases share a
    pressure grid; else the host functions per case."""
    if all(d is None for d in decks):
        return
    if any(d is None for d in decks):
        raise Exception("MODEL: some rows of the batch have clouds and others have none")
    kinds = {kind for sample in decks for kind, _ in sample}
    p0 = np.asarray(cases[0].inputs['atmosphere']['profile']['pressure'])
    same_grid = all(np.array_equal(p0, np.asarray(c.inputs['atmosphere']['profile']['pressure'])) for c in cases[1:])
    family = _GREY if kinds <= set(_GREY) else (_MIE if kinds <= set(_MIE) else None)
    if family is None or not same_grid or not all(1 <= len(sample) <= 4 for sample in decks):
        for A, sample, cfg in zip(cases, decks, configs):
            param_tools.add_class(A)
            A.clouds(df=cloud_averaging([_cloud_host(kind, kw, cfg, param_tools) for kind, kw in sample]))
        return
    param_tools.add_class(cases[0])
    records = [[_deck_record(kind, kw, cfg) for kind, kw in sample] for sample, cfg in zip(decks, configs)]
    if family is _GREY:
        tables = param_tools.cloud_tables_batch(records, average=1)
    else:
        from . import mie
        tables = mie.cloud_tables_batch(param_tools, records, average=1)
    for A, table in zip(cases, tables):
        A.clouds(df=table)


def MODEL(cube, fitpars, config, OPA, param_tools, DATA_DICT, retrieval=True):
    """The model of every row of ``cube`` (``(ndim,)`` or ``(N, ndim)``) on the grid of every data set:
    ``{instrument: (N, ndata)}``, and with ``retrieval=False`` also ``{row: profile}`` (reference driver.py:176-251).
    ``thermal``: ``1e-8 (R / d)^2 out['thermal']``; ``transmission``: ``out['transit_depth']``.  ``reflected`` raises: the
    reference's ``MODEL`` forms every model from ``out['thermal']`` and so defines no reflected branch.  One launch per
    stage for the whole cube (the module's docstring); the caller's ``config`` is not modified (the reference leaves the
    last row's values in it)."""
    obs_type = config['observation_type']
    if obs_type == 'reflected':
        raise NotImplementedError("MODEL(observation_type='reflected'): the reference's MODEL forms every model from "
                                  "out['thermal'] (driver.py:230) and so defines no reflected branch; there is nothing to "
                                  "reproduce")
    if obs_type not in ('thermal', 'transmission'):
        raise Exception("MODEL: observation_type is 'thermal' or 'transmission', got %r" % (obs_type,))
    cube = np.atleast_2d(cube)
    names = list(config['InputOutput']['observation_data'])
    base = _regrid.instruments_plan(OPA, _instruments(config, DATA_DICT))
    cases, visscher, decks, configs, plans = [], [], [], [], []
    for row in cube:
        cfg = _copy_config(config)
        for i, key in enumerate(fitpars.keys()):
            if not key.startswith(_NOT_MODEL):
                set_dict_value(cfg, key + ".value", row[i])
        A, vis = _setup_base(cfg, OPA, param_tools)
        cases.append(A), visscher.append(vis), decks.append(_cloud_decks(cfg)), configs.append(cfg)
        plans.append(base.with_scale(_flux_scale(cfg)) if obs_type == 'thermal' else base)
    todo = [j for j, v in enumerate(visscher) if v is not None]
    if todo:
        _chem_visscher([cases[j] for j in todo], [visscher[j] for j in todo])
    _batch_clouds(cases, decks, configs, param_tools)
    outs = jdi.spectrum_batch(cases, OPA, calculation=obs_type, instruments=plans)
    leg = 'thermal' if obs_type == 'thermal' else 'transit_depth'
    y_model = {key: np.vstack([out[leg][base.slices[key]] for out in outs]) for key in names}
    if retrieval:
        return y_model
    return y_model, {j: A.inputs['atmosphere']['profile'] for j, A in enumerate(cases)}


def log_likelihood(cube, fitpars, config, OPA, DATA_DICT, param_tools):
    """The log-likelihood of every row of ``cube``: a scalar for one row, ``(N,)`` otherwise (reference driver.py:253-332).
    ``MODEL`` for the whole cube, then per row, over the data sets in ``observation_data`` order, concatenated:
    ``ydata_ = (ydata + offset) * scaling``, ``sigma = edata**2 + err_inf``,
    ``-0.5 * np.sum((ydata_ - ymod)**2 / sigma + np.log(2 pi sigma))``, with ``offset.<name>``, ``scaling.<name>`` and
    ``err_inf.<name>`` read from the cube by their place in ``fitpars``.  Host numpy in the reference's operation order."""
    cube = np.atleast_2d(cube)
    models = MODEL(cube, fitpars, config, OPA, param_tools, DATA_DICT)
    names = list(config['InputOutput']['observation_data'])
    place = {key: i for i, key in enumerate(fitpars.keys())}
    nuisance = config.get("retrieval", {})

    def fitted(row, kind, name, absent):
        """``<kind>.<name>`` of this row where the configuration fits one, else the value that changes nothing."""
        return row[place["%s.%s" % (kind, name)]] if name in nuisance.get(kind, {}) else absent

    def terms(row, name):
        """One data set of one row: the shifted and scaled data, the variance and its normalisation term."""
        ydata, edata = DATA_DICT[name][1], DATA_DICT[name][2]
        shifted = (ydata + fitted(row, "offset", name, 0)) * fitted(row, "scaling", name, 1)
        variance = edata ** 2 + fitted(row, "err_inf", name, 0)
        return shifted, variance, np.log(2 * np.pi * variance)
    out = np.empty(cube.shape[0])
    for j, row in enumerate(cube):
        data, variance, norm = (np.concatenate(part) for part in zip(*(terms(row, name) for name in names)))
        model = np.concatenate([models[name][j] for name in names])
        out[j] = -0.5 * np.sum((data - model) ** 2 / variance + norm)      # one sum over all data sets, as the reference
    return out[0] if cube.shape[0] == 1 else out


def make_loglike(config, OPA, DATA_DICT, param_tools):
    """``(loglike_fn, prior_fn, fitpars)``: the two ``partial``s the reference's ``retrieve`` hands to its sampler
    (driver.py:392-403), for any sampler's vectorised interface -- ``loglike_fn((N, ndim))`` is ``(N,)``,
    ``prior_fn((N, ndim))`` is ``(N, ndim)``."""
    fitpars = prior_finder(config['retrieval'])
    loglike_fn = partial(log_likelihood, fitpars=fitpars, config=config, OPA=OPA, param_tools=param_tools,
                         DATA_DICT=DATA_DICT)
    return loglike_fn, partial(hypercube, fitpars=fitpars), fitpars


def _opannection(config):
    op = config['OpticalProperties']
    return jdi.opannection(filename_db=op['opacity_files'], method=op['opacity_method'], **op.get('opacity_kwargs', {}))


def check_model_samples(config, N=100, samples=None, OPA=None):
    """Models of ``N`` draws from the prior, or of the first ``N`` of ``samples`` (reference driver.py:429-482):
    ``(models, thetas, profiles)``.  ``OPA``: an opacity object to use instead of opening
    ``config['OpticalProperties']``."""
    fitpars = prior_finder(config['retrieval'])
    if samples is None:
        samples = hypercube(np.random.random([N, len(fitpars)]), fitpars)       # row by row the reference's draws
    thetas = np.array(samples)
    models, profiles = MODEL(thetas[:N], fitpars, config, _opannection(config) if OPA is None else OPA, Parameterize(),
                             get_data(config), retrieval=False)
    return models, thetas, profiles


def _read_toml(driver_file):
    for name in ("tomllib", "tomli"):
        try:
            toml = __import__(name)
        except ImportError:
            continue
        with open(driver_file, "rb") as f:
            return toml.load(f)
    raise ImportError("run(driver_file=%r): a TOML file is read with tomllib (Python 3.11) or tomli, and neither is "
                      "installed; read the file yourself and pass driver_dict=" % (driver_file,))


def run(driver_file=None, driver_dict=None):
    """Run a configuration (reference driver.py:28-71).  ``calc_type = 'spectrum'``: ``setup_spectrum_class`` and
    ``spectrum(full_output=True)``.  ``'retrieval'``: what ``make_loglike`` returns -- this package installs and starts no
    sampler; hand the two functions to one."""
    if isinstance(driver_file, str):
        config = _read_toml(driver_file)
    elif isinstance(driver_dict, dict):
        config = driver_dict
    else:
        raise Exception('Could not interpret either driver file or dictionary input')
    kind = config['calc_type']
    if kind not in ('spectrum', 'retrieval'):
        raise Exception("run: calc_type is 'spectrum' or 'retrieval', got %r (a climate run is set up with "
                        "inputs.setup_climate(), not from a configuration)" % (kind,))
    param_tools, opacity = Parameterize(), _opannection(config)
    if kind == 'retrieval':
        return make_loglike(config, opacity, get_data(config), param_tools)
    case = setup_spectrum_class(config, opacity, param_tools)
    return case.spectrum(opacity, full_output=True, calculation=config['observation_type'])
