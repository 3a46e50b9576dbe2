"""CPU-only checks of the batched cloud path: the NumPy mirror of the deck state
(continuum.deck_state, what pb_deck_state_batch computes per walker) against fixture G11 and
against continuum.Deck, the cloud-type bookkeeping of Continuum(cloud_models=...), and the new
entry points' argument checks, which come before any HIP call."""
import ctypes as C

import numpy as np
import pytest

RTS = ['transit', 'emission', 'eclipse']


@pytest.mark.parametrize('rt', RTS)
def test_deck_state_reproduces_g11(golden, rt):
    """The reference's own deck state (gray.py:129-150): itop, rsurf, tsurf of `deck -3.0`."""
    from pyratbay_amd import continuum as ct
    g = golden('g11_patchy')
    logp, itop, rsurf, tsurf = g[f'{rt}_deck']
    got = ct.deck_state(g[f'{rt}_press'], [logp], g[f'{rt}_radius'], g[f'{rt}_temp'][None])
    assert got[0].dtype == np.int32 and int(got[0][0]) == int(itop)
    np.testing.assert_allclose(got[1][0], rsurf, rtol=1e-13)
    np.testing.assert_allclose(got[2][0], tsurf, rtol=1e-13)


def test_deck_state_equals_deck_model():
    """Per walker the mirror is continuum.Deck.calc_extinction_coefficient, beyond both ends of
    the pressure grid and on a grid pressure included; shared and per-walker radius."""
    from pyratbay_amd import continuum as ct
    rng = np.random.default_rng(4)
    L, nw = 23, 40
    pressure = np.logspace(-6, 2, L)
    logp = rng.uniform(-7.5, 3.5, nw)
    logp[:4] = [-9.0, 5.0, np.log10(pressure[7]), 2.0]
    temps = rng.uniform(500, 2500, (nw, L))
    radius = np.linspace(8e9, 7e9, L) * (1 + 0.02 * rng.uniform(-1, 1, (nw, 1)))
    itop, rsurf, tsurf = ct.deck_state(pressure, logp, radius, temps)
    itop1, rsurf1, _ = ct.deck_state(pressure, logp, radius[:1], temps)
    deck = ct.Deck(pressure, np.linspace(1000, 2000, 5))
    for w in range(nw):
        want = deck.calc_extinction_coefficient(radius[w], temps[w], [logp[w]])
        assert (int(itop[w]), rsurf[w], tsurf[w]) == want
        assert (int(itop1[w]), rsurf1[w]) == deck.calc_extinction_coefficient(
            radius[0], temps[w], [logp[w]])[:2]
    assert itop[0] == 1 and rsurf[0] == radius[0, 0] and tsurf[0] == temps[0, 0]
    assert itop[1] == L - 1 and rsurf[1] == radius[1, -1] and tsurf[1] == temps[1, -1]
    assert itop[2] == 7 and itop[3] == L - 1
    assert set(itop.tolist()) >= {1, L - 1} and len(set(itop.tolist())) > 5


def test_cloud_models_bookkeeping():
    """species and free_pars do not depend on what is cloud-type; only Lecavelier, CCSgray and the
    Deck may be; the default is today's: no cloud-type model."""
    from pyratbay_amd import continuum as ct
    wn = np.linspace(1000.0, 2000.0, 50)
    pressure = np.logspace(-6, 2, 12)
    ray, lec = ct.Kurucz(wn, 'H2'), ct.Lecavelier(pressure, wn=wn)
    gray, deck, he = ct.CCSgray(pressure, wn), ct.Deck(pressure, wn), ct.Kurucz(wn, 'He')
    sodium = ct.SodiumVdW(pressure, wn=wn)
    models = [ray, lec, he, gray, deck]
    pars = [('lecavelier', 0), ('lecavelier', 1), ('ccsgray', 0), ('ccsgray', 1), ('ccsgray', 2)]
    plain = ct.Continuum(wn, pressure, models)
    assert plain.cloud == [] and plain.species == ['H2', 'He'] and plain.free_pars == pars
    assert plain.batch_unsupported() == ['deck'] and plain.batch_unsupported(deck=True) == []
    cont = ct.Continuum(wn, pressure, models, cloud_models=[gray, deck, lec])
    assert cont.cloud == [lec, gray]                          # model order, the deck is no term
    assert cont.species == ['H2', 'He'] and cont.free_pars == pars
    assert cont._par_offsets() == [0, 0, 2, 2] and cont.is_cloud(lec) and not cont.is_cloud(ray)
    assert ct.Continuum(wn, pressure, models, cloud_models=[gray]).cloud == [gray]
    with pytest.raises(ValueError, match='cannot be cloud-type'):
        ct.Continuum(wn, pressure, models, cloud_models=[ray])
    with pytest.raises(ValueError, match='cannot be cloud-type'):
        ct.Continuum(wn, pressure, models + [sodium], cloud_models=[sodium])
    with pytest.raises(ValueError, match='one of the models'):
        ct.Continuum(wn, pressure, models, cloud_models=[ct.Lecavelier(pressure, wn=wn)])


def test_entry_points_check_arguments_first():
    from pyratbay_amd import _capi
    from pyratbay_amd.continuum import CloudModelsStruct, CloudTermsStruct
    fake = C.c_void_p(16)          # never dereferenced: the checks come first
    for name in ('pb_deck_state_batch', 'pb_cloud_plan', 'pb_cloudy_transit_batch',
                 'pb_cloudy_emission_batch'):
        assert name in _capi.exported_names() and hasattr(_capi.lib(), name)
    with pytest.raises(_capi.PbError, match='radius_stride'):
        _capi.call('pb_deck_state_batch', fake, fake, fake, fake, fake, fake, 5, fake, 12, 4, None)
    terms = CloudTermsStruct()
    terms.nr = 9
    transit = [fake] * 5 + [0, fake, 0, None, 1e10, 0, 10.0, 12, 100, 4]
    with pytest.raises(_capi.PbError, match='cloud terms'):
        _capi.call('pb_cloudy_transit_batch', *transit, None, None, C.byref(terms), None, None)
    with pytest.raises(_capi.PbError, match='go together'):
        _capi.call('pb_cloudy_transit_batch', *transit, fake, None, None, None, None)
    transit[10] = 12
    with pytest.raises(_capi.PbError, match='itop out of range'):
        _capi.call('pb_cloudy_transit_batch', *transit, None, None, None, None, None)
    emission = [fake] * 9 + [None, 17, 10.0, 0, 12, 100, 4]
    with pytest.raises(_capi.PbError, match='nmu'):
        _capi.call('pb_cloudy_emission_batch', *emission, None, None, None, None, None)
    models = CloudModelsStruct()
    models.nr, models.kind[0] = 1, 0
    with pytest.raises(_capi.PbError, match='kind 1'):
        _capi.call('pb_cloud_plan', fake, fake, C.byref(models), fake, fake, 0, fake, 12, 100, 4,
                   None)
