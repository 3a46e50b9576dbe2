"""Band contribution functions, the parts that need no GPU: the NumPy statements of
pyratbay_amd/contribution.py against the reference's own results (tests/golden/
g24_contribution.npz, written by make_golden_contribution.py from the unmodified
spectrum/contribution_funcs.py), the plan of an eval_bands call that asks for them, the argument
refusals that happen before the device is touched, and the new field of PosteriorSummary."""
import itertools
import os

import numpy as np
import pytest

from pyratbay_amd import contribution as cb
from pyratbay_amd import posterior
from pyratbay_amd.table import plan_eval_bands

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def g24():
    return np.load(os.path.join(HERE, 'golden', 'g24_contribution.npz'))


def case_names():
    with np.load(os.path.join(HERE, 'golden', 'g24_contribution.npz')) as g:
        return [str(c) for c in g['cases']]


def load_case(g, name):
    """The arrays of one case and its bands as (responses, indices)."""
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + '_')}
    W = len(c['wn'])
    start, count = g[f'W{W}_band_start'], g[f'W{W}_band_count']
    offs = np.concatenate([[0], np.cumsum(count)])
    c['responses'] = [g[f'W{W}_response'][offs[b]:offs[b + 1]] for b in range(len(start))]
    c['indices'] = [np.arange(start[b], start[b] + count[b]) for b in range(len(start))]
    c['rt'] = str(c['rt'])
    return c


def close(got, want):
    """Bit-equal or within 4 eps (relative), and the same NaN pattern."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 4 * EPS * np.abs(want[ok]))


@pytest.mark.parametrize('name', case_names())
def test_host_forms_against_reference(g24, name):
    c = load_case(g24, name)
    nw = c['depth'].shape[0]
    for w in range(nw):
        if c['rt'] == 'transit':
            contrib = cb.transmittance_host(c['depth'][w], c['ideep'][w])
        else:
            contrib = cb.contribution_function_host(c['depth'][w], c['press'], c['planck'][w])
        close(contrib, c['contrib'][w])
        close(cb.band_cf_host(contrib, c['responses'], c['wn'], c['indices']), c['band'][w])
        close(cb.band_contribution_host(c['depth'][w], c['ideep'][w], c['responses'], c['wn'],
                                        c['indices'], rt_path=c['rt'], pressure=c['press'],
                                        planck=c.get('planck', [None] * nw)[w]), c['band'][w])


def test_fixture_covers_what_it_claims(g24):
    """The band of one sample is NaN in every layer and nothing else is; the small-maxdepth case
    has kept and zeroed jumps; L = 2 results are exactly 1 and 0."""
    for name in case_names():
        c = load_case(g24, name)
        single = np.array([len(r) == 1 for r in c['responses']])
        assert single.any() and np.all(np.isnan(c['band'][:, :, single]))
        assert np.all(np.isfinite(c['band'][:, :, ~single]))
        assert float(c['sens']) <= 1e-9
    c = load_case(g24, 'e_md')
    jump = np.diff(np.exp(-c['depth'][0]), axis=0)
    assert np.any((jump > 0) & (jump <= 0.1)) and np.any(jump > 0.1)
    for name in ('t_l2', 'e_l2'):
        c = load_case(g24, name)
        single = np.array([len(r) == 1 for r in c['responses']])
        assert np.all(c['band'][0, 0, ~single] == 1.0) and np.all(c['band'][0, 1, ~single] == 0.0)


def test_host_forms_leave_their_inputs_alone(g24):
    c = load_case(g24, 't_l9')
    depth = c['depth'][0].copy()
    cb.transmittance_host(depth, c['ideep'][0])
    assert np.array_equal(depth, c['depth'][0])


def test_band_contribution_host_needs_pressure_and_planck(g24):
    c = load_case(g24, 'e_l3')
    with pytest.raises(ValueError, match='pressure and planck'):
        cb.band_contribution_host(c['depth'][0], c['ideep'][0], c['responses'], c['wn'],
                                  c['indices'], rt_path='emission')


@pytest.mark.parametrize('rt_path', ['transit', 'emission', 'two_stream'])
def test_plan_with_contribution_never_orders(rt_path):
    """With the fact `contribution` the plan has no column order, no layer limits, no one-pass
    form and no auto ordering, whatever the model's facts are; without it (absent or False)
    nothing changes."""
    for nrows, itop, nwave in itertools.product([1, 2, 40, 128, 129], [0, 3], [1, 2, 64, 600]):
        for order, limit, one_pass, continuum in itertools.product([False, True], repeat=4):
            facts = dict(rt_path=rt_path, nlayers=nrows + itop, itop=itop, nwave=nwave,
                         order_set=order, tile_limit_set=limit, one_pass=one_pass,
                         continuum=continuum)
            got = plan_eval_bands(facts, dict(cloudy=False, contribution=True))
            assert got.form == rt_path
            assert got.ordered is False and got.limited is False
            assert (got.table, got.wn, got.column) == ('etable', 'wn', None)
            assert got.may_auto_order is False
            assert plan_eval_bands(facts, dict(cloudy=False, contribution=False)) == \
                plan_eval_bands(facts, dict(cloudy=False))


def test_posterior_summary_field():
    """The new field is last and defaults to None."""
    assert posterior.PosteriorSummary._fields[-1] == 'contribution'
    s = posterior.PosteriorSummary(1, 2, 3, 4, 5, 6, 7)
    assert s.contribution is None and s.stores == 7


def test_engine_reexports():
    import pyratbay_amd.engine as engine
    for name in ('contribution', 'transmittance_host', 'contribution_function_host',
                 'band_cf_host', 'band_contribution_host', 'band_transmittance_batch',
                 'band_contribution_emission_batch'):
        assert getattr(engine, name, None) is not None, name


def test_capi_declares_the_entries():
    """The three entries are in the header, the binding and the library; the work size follows
    parts[nw, nbands, ceil(max count / 256), L], and is 0 for an empty call."""
    from pyratbay_amd import _capi
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'pbhip.h')).read()
    for name in ('pb_band_contribution_emission_batch', 'pb_band_transmittance_batch',
                 'pb_band_contribution_work_doubles'):
        assert name in text and name in _capi.exported_names() and hasattr(_capi.lib(), name)
    f = _capi.lib().pb_band_contribution_work_doubles
    assert f(40, 10, 513, 3) == 3 * 10 * 3 * 40
    assert f(40, 10, 256, 3) == 3 * 10 * 1 * 40
    assert f(40, 10, 257, 3) == 3 * 10 * 2 * 40
    assert f(40, 0, 257, 3) == 0 and f(40, 10, 257, 0) == 0 and f(40, 10, 0, 3) == 0


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """Argument checks come before any HIP call: they answer PB_ERR_ARG without a GPU; zero
    walkers or zero bands succeed."""
    from pyratbay_amd import _capi
    lib = _capi.lib()
    one = 8                                         # (never dereferenced: a non-null pointer value)
    def emission(nlayers=4, nwave=8, nbands=2, nw=1, itop=0, ibottom=4, out=one, work=one):
        return lib.pb_band_contribution_emission_batch(
            out, one, one, one, one, one, one, one, one, one, 300, 10.0, itop, ibottom, nlayers,
            nwave, nbands, nw, work, None)

    def transit(nlayers=4, nwave=8, nbands=2, nw=1, itop=0, out=one, work=one):
        return lib.pb_band_transmittance_batch(out, one, one, one, one, one, one, one, 300, itop,
                                               nlayers, nwave, nbands, nw, work, None)
    assert emission(nw=0) == 0 and emission(nbands=0) == 0
    assert transit(nw=0) == 0 and transit(nbands=0) == 0
    for bad in (dict(nlayers=1), dict(nlayers=1025), dict(itop=4), dict(itop=-1),
                dict(ibottom=5), dict(nwave=0), dict(nw=-1), dict(out=None), dict(work=None),
                dict(nbands=65536)):
        assert emission(**bad) != 0, bad
        assert b'pb_band_contribution_emission_batch' in lib.pb_last_error()
    for bad in (dict(nlayers=0), dict(nlayers=2049), dict(itop=4), dict(itop=-1), dict(nwave=0),
                dict(nw=-1), dict(out=None), dict(work=None), dict(nw=65536)):
        assert transit(**bad) != 0, bad
        assert b'pb_band_transmittance_batch' in lib.pb_last_error()
