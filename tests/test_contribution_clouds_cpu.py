"""Band contribution functions with clouds, the parts that need no GPU: the NumPy statements
contribution.transmittance_patchy_host / band_contribution_cloudy_host against the reference's own
results (tests/golden/g27_contribution_clouds.npz, written by make_golden_contribution_clouds.py
from the unmodified package), the fixture's stored preconditions, the plan of a cloudy
contribution call, the exported symbols, and the argument refusals of the two new entries that
happen before the device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from pyratbay_amd import contribution as cb
from pyratbay_amd.table import plan_eval_bands

HERE = os.path.dirname(os.path.abspath(__file__))
G27 = os.path.join(HERE, 'golden', 'g27_contribution_clouds.npz')


@pytest.fixture(scope='module')
def g27():
    return np.load(G27)


def case_names():
    with np.load(G27) as g:
        return [str(c) for c in g['cases']]


def load_case(g, name):
    """The arrays of one case, its bands as (responses, indices) and the bands' device arrays."""
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + '_')}
    W = len(c['wn'])
    start, count = g[f'W{W}_band_start'], g[f'W{W}_band_count']
    offs = np.concatenate([[0], np.cumsum(count)])
    c['band_start'], c['band_count'], c['response'] = start, count, g[f'W{W}_response']
    c['response_offset'] = offs[:-1].astype(np.int64)
    c['responses'] = [c['response'][offs[b]:offs[b + 1]] for b in range(len(start))]
    c['indices'] = [np.arange(start[b], start[b] + count[b]) for b in range(len(start))]
    c['rt'] = str(c['rt'])
    c['sens'] = float(c['sens'])
    c['single'] = np.array([len(r) == 1 for r in c['responses']])
    return c


def bound(c):
    """The project's rule (contribution_cases.bound): max(10 sens, 1e-14), absolute, on the
    max-normalised result."""
    return max(10 * c['sens'], 1e-14)


def host_band(c, w):
    """band_contribution_cloudy_host on walker w of a case, with the clamped fraction."""
    kw = {}
    if 'f_clamped' in c:
        kw['f_patchy'] = c['f_clamped'][w]
    if 'depth_clear' in c:
        kw.update(depth_clear=c['depth_clear'][w], ideep_clear=c['ideep_clear'][w])
    if c['rt'] != 'transit':
        kw.update(pressure=c['press'], planck=c['planck'][w])
    return cb.band_contribution_cloudy_host(c['depth'][w], c['ideep'][w], c['responses'], c['wn'],
                                            c['indices'], rt_path=c['rt'], **kw)


def assert_within(got, want, c, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN pattern'
    ok = ~np.isnan(want)
    worst = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
    print(f'{what}: largest difference {worst:.2e}, bound {bound(c):.2e}')
    assert worst <= bound(c), f'{what}: {worst:.2e} > {bound(c):.2e}'


@pytest.mark.parametrize('name', case_names())
def test_host_forms_against_reference(g27, name):
    c = load_case(g27, name)
    for w in range(c['depth'].shape[0]):
        assert_within(host_band(c, w), c['band'][w], c, f'{name} walker {w}')
        if c['rt'] == 'transit' and 'f_clamped' in c:
            contrib = cb.transmittance_patchy_host(c['depth'][w], c['ideep'][w],
                                                   c['depth_clear'][w], c['ideep_clear'][w],
                                                   c['f_clamped'][w])
            assert np.max(np.abs(contrib - c['contrib'][w])) <= 4 * np.finfo(float).eps


def test_emission_ignores_the_clear_column_and_the_fraction(g27):
    """As the reference: depth_clear, ideep_clear and f_patchy change nothing in emission."""
    c = load_case(g27, 'e_mid')
    plain = cb.band_contribution_cloudy_host(c['depth'][0], c['ideep'][0], c['responses'],
                                             c['wn'], c['indices'], rt_path='emission',
                                             pressure=c['press'], planck=c['planck'][0])
    given = cb.band_contribution_cloudy_host(c['depth'][0], c['ideep'][0], c['responses'],
                                             c['wn'], c['indices'], rt_path='emission',
                                             depth_clear=c['depth'][0] * 0.5,
                                             ideep_clear=c['ideep'][0], f_patchy=0.37,
                                             pressure=c['press'], planck=c['planck'][0])
    assert np.array_equal(plain, given, equal_nan=True)
    with pytest.raises(ValueError, match='pressure and planck'):
        cb.band_contribution_cloudy_host(c['depth'][0], c['ideep'][0], c['responses'], c['wn'],
                                         c['indices'], rt_path='emission')
    t = load_case(g27, 't_mid')
    with pytest.raises(ValueError, match='depth_clear'):
        cb.band_contribution_cloudy_host(t['depth'][0], t['ideep'][0], t['responses'], t['wn'],
                                         t['indices'], f_patchy=0.37)


def test_fixture_covers_what_it_claims(g27):
    """The preconditions the generator asserted, read back from what it stored."""
    names = case_names()
    for name in names:
        c = load_case(g27, name)
        assert c['single'].any() and np.all(np.isnan(c['band'][:, :, c['single']]))
        assert np.all(np.isfinite(c['band'][:, :, ~c['single']]))
        assert np.all(np.isfinite(c['contrib'])) and c['sens'] <= 1e-9
        assert np.all(np.diff(c['wn']) > 0) and np.ptp(np.diff(c['wn'])) > 0.5   # non-uniform
    counts = sorted(set(load_case(g27, 't_l40')['band_count'].tolist()))
    assert {1, 2, 255, 256, 257, 513} <= set(counts)
    # transit: the deck's layer per case
    want = {'t_l2': [1], 't_l3': [1], 't_top': [1, 2], 't_next': [3], 't_mid': [5], 't_bot': [8],
            't_l40': [17], 'e_next': [3], 'e_mid': [5], 'e_bot': [8], 'e_bot2': [7]}
    for name, decks in want.items():
        assert load_case(g27, name)['deck_itop'].tolist() == decks, name
    assert 'deck_itop' not in load_case(g27, 't_nodeck') and 'cloud_f' in load_case(g27, 't_nodeck')
    assert 'deck_itop' not in load_case(g27, 'e_nodeck') and 'cloud_f' in load_case(g27, 'e_nodeck')
    c = load_case(g27, 't_top')                      # no cloudy row: 0 from itop on, 1 above
    itop = int(c['itop'])
    assert np.all(c['ideep'] == itop) and np.all(c['depth'] == 0)
    assert np.all(cb.transmittance_host(c['depth'][0], c['ideep'][0])[itop:] == 0)
    assert np.all(c['contrib'][0][:itop] == 1.0)
    c = load_case(g27, 't_w3')
    assert c['depth'].shape[0] == 3 and len(set(c['deck_itop'].tolist())) == 3
    assert len(set(c['f_patchy'].tolist())) == 3 and not np.array_equal(c['radius'][0],
                                                                       c['radius'][1])
    fractions = np.concatenate([load_case(g27, n).get('f_patchy', np.zeros(0)) for n in names
                                if n.startswith('t_')])
    assert {0.0, 1.0, 0.37} <= set(fractions.tolist())
    assert np.any((fractions < 0) | (fractions > 1))
    c = load_case(g27, 't_bot')
    assert c['f_patchy'][0] == 1.4 and c['f_clamped'][0] == 1.0
    for name in ('t_mid', 't_l40'):
        c = load_case(g27, name)
        dk, md, cols = int(c['deck_itop'][0]), float(c['maxdepth']), np.arange(len(c['wn']))
        by_depth = c['depth'][0][c['ideep'][0], cols] > md
        assert np.any(by_depth & (c['ideep'][0] < dk)) and np.any(~by_depth & (c['ideep'][0] == dk))
        assert np.any(c['ideep'][0] < c['ideep_clear'][0])
        assert np.any(~(c['depth_clear'][0][c['ideep_clear'][0], cols] > md))
    c = load_case(g27, 't_l40')
    assert c['depth'].shape[1:] == (40, 600) and (40 - int(c['itop'])) % 16 != 0
    for name in ('e_next', 'e_mid', 'e_bot2', 'e_md'):
        c = load_case(g27, name)
        dk = int(c['deck_itop'][0])
        assert np.any(c['ideep'][0] == dk + 1) and np.any(c['ideep'][0] <= dk)
        assert np.all(c['depth'][0][dk + 2:] == 0)
        assert abs(c['deck_tsurf'][0] - c['temps'][0, dk]) > 50.0
    c = load_case(g27, 'e_md')
    jump = np.diff(np.exp(-c['depth'][0]), axis=0)
    assert np.any((jump > 0) & (jump <= 0.1)) and np.any(jump > 0.1)
    assert os.path.getsize(G27) <= os.path.getsize(os.path.join(HERE, 'golden',
                                                                'g24_contribution.npz'))


def test_cloud_factors_rebuild_ec_cloud(g27):
    """The rank-1 factors the device entries take give the cloudy column the depth was made of:
    the plane-parallel depth of ec + sum_m cs_m f_m matches the stored one."""
    c = load_case(g27, 'e_nodeck')
    ecc = c['ec'][0] + sum(c['cloud_f'][0, :, m, None] * c['cloud_cs'][m, 0] for m in range(2))
    h = -np.diff(c['radius'][0])
    itop, L = int(c['itop']), len(c['press'])
    acc = np.zeros(len(c['wn']))
    open_ = np.ones(len(c['wn']), bool)
    for k in range(itop + 1, L):
        acc = acc + 0.5 * h[k - 1] * (ecc[k] + ecc[k - 1])
        got = np.where(open_, acc, 0.0)
        assert np.allclose(got, c['depth'][0][k], rtol=1e-13, atol=0.0)
        open_ &= ~(acc >= float(c['maxdepth']))


@pytest.mark.parametrize('rt_path', ['transit', 'emission'])
def test_plan_of_a_cloudy_contribution_call(rt_path):
    """Grid order, every layer, no auto ordering, the cloud form."""
    for order, limit, one_pass in ((False, False, False), (True, True, True)):
        facts = dict(rt_path=rt_path, nlayers=40, itop=0, nwave=600, order_set=order,
                     tile_limit_set=limit, one_pass=one_pass, continuum=True)
        got = plan_eval_bands(facts, dict(cloudy=True, contribution=True))
        assert got.form == 'clouds' and got.ordered is False and got.limited is False
        assert (got.table, got.wn, got.column) == ('etable', 'wn', None)
        assert got.may_auto_order is False


def test_symbols_exported_and_declared():
    import pyratbay_amd.engine as engine
    from pyratbay_amd import _capi, batch
    for name in ('transmittance_patchy_host', 'band_contribution_cloudy_host'):
        assert name in cb.__all__ and getattr(engine, name) is getattr(cb, name)
    for name in ('band_transmittance_cloudy_batch', 'band_contribution_emission_cloudy_batch'):
        assert getattr(engine, name) is getattr(batch, name)
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'pbhip.h')).read()
    for name in ('pb_band_transmittance_cloudy_batch',
                 'pb_band_contribution_emission_cloudy_batch'):
        assert name in text and name in _capi.exported_names() and hasattr(_capi.lib(), name)
    assert 'PB_BAND_CLOUDY_MAX_LAYERS 400' in text


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """Argument checks come before any HIP call: they answer PB_ERR_ARG without a GPU, with the
    entry's name in pb_last_error(); zero walkers or zero bands succeed."""
    from pyratbay_amd import _capi
    from pyratbay_amd.continuum import CloudTermsStruct
    lib = _capi.lib()
    one = 8                                         # (never dereferenced: a non-null pointer value)
    terms = CloudTermsStruct()
    terms.nr, terms.f_d = 9, one                    # PB_CLOUD_MAX is 8
    no_factors = CloudTermsStruct()
    no_factors.nr = 2

    def emission(nlayers=4, nwave=8, nbands=2, nw=1, itop=0, ibottom=4, out=one, work=one,
                 deck_itop=one, deck_tsurf=one, cloud=None):
        return lib.pb_band_contribution_emission_cloudy_batch(
            out, one, one, one, one, one, one, one, one, one, 300, 10.0, itop, ibottom, nlayers,
            nwave, nbands, nw, deck_itop, deck_tsurf,
            None if cloud is None else C.byref(cloud), work, None)

    def transit(nlayers=4, nwave=8, nbands=2, nw=1, itop=0, out=one, work=one, stride=6,
                cloud=None):
        return lib.pb_band_transmittance_cloudy_batch(
            out, one, one, stride, one, one, one, one, one, 300, itop, 10.0, nlayers, nwave,
            nbands, nw, one, None if cloud is None else C.byref(cloud), one, work, None)
    assert emission(nw=0) == 0 and emission(nbands=0) == 0
    assert transit(nw=0) == 0 and transit(nbands=0) == 0
    for bad in (dict(nlayers=1), dict(nlayers=1025), dict(itop=4), dict(itop=-1),
                dict(ibottom=5), dict(nwave=0), dict(nw=-1), dict(out=None), dict(work=None),
                dict(nbands=65536), dict(deck_tsurf=None), dict(deck_itop=None),
                dict(cloud=terms), dict(cloud=no_factors)):
        assert emission(**bad) != 0, bad
        assert b'pb_band_contribution_emission_cloudy_batch' in lib.pb_last_error(), bad
    for bad in (dict(nlayers=0), dict(nlayers=401, stride=0), dict(itop=4), dict(itop=-1),
                dict(nwave=0), dict(nw=-1), dict(out=None), dict(work=None), dict(nw=65536),
                dict(stride=5), dict(cloud=terms), dict(cloud=no_factors)):
        assert transit(**bad) != 0, bad
        assert b'pb_band_transmittance_cloudy_batch' in lib.pb_last_error(), bad
    assert b'400' in (transit(nlayers=401, stride=0), lib.pb_last_error())[1]
    assert b'cloud terms' in (transit(cloud=terms), lib.pb_last_error())[1]
