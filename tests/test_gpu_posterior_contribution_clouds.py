"""posterior_summary(..., contribution=True, deck_logp=, f_patchy=): the median over the chain of
the band contribution functions of a cloudy retrieval (tools/retrieval_tools.py:474-504 on
Pyrat.band_contribution's cloudy form, pyrat_obj.py:671-696), on the shape of
test_gpu_posterior_contribution.py -- five unique samples with counts [3, 1, 4, 1, 2] in chunks of
2, a Continuum with a Deck (beside Rayleigh, CIA, H- and the alkali doublets), each sample with
its own deck pressure and cloudy fraction -- and one sample the batch rejects.  Equal bits
throughout."""
import numpy as np
import pytest

import test_gpu_posterior as tpost
from pyratbay_amd import posterior as post

pytestmark = pytest.mark.gpu

COUNTS, CHUNK = tpost.COUNTS, tpost.CHUNK


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def pa():
    from pyratbay_amd import atmosphere
    return atmosphere


@pytest.fixture(scope='module')
def g7(golden):
    return golden('g7_continuum')


def host(t):
    return t.cpu().numpy()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('geometry', ['transit_clouds', 'emission_clouds'])
def test_posterior_contribution_with_clouds(eng, pa, g7, geometry):
    import torch
    model, atm, params, pb, kw, hot = tpost.atmosphere_case(eng, pa, g7, geometry)
    assert 'deck_logp' in kw and 'f_patchy' in kw and model.continuum.deck
    chain = np.repeat(params, COUNTS, axis=0)[np.random.default_rng(1).permutation(COUNTS.sum())]
    u_index, counts, inverse = post.unique_samples(chain)
    unique = eng.dev(chain[u_index])
    L, nb = model.nlayers, pb.nbands
    res = model.posterior_summary(atm, unique, counts, pb, chunk=CHUNK, keep_stores=True,
                                  contribution=True, **kw)
    assert res.n_rejected == 0 and res.contribution.shape == (L, nb)
    store = res.stores['contribution']
    assert store.shape == (L, nb, 5)
    cf = np.moveaxis(host(store), -1, 0)                       # [n, L, nbands]
    finite = np.isfinite(cf).all(axis=(0, 1))
    assert finite.any()                                        # (not every band has one sample)
    assert np.all(cf[:, :, finite].max(axis=1) == 1.0)
    # the median has np.median's bits over the expanded chain (11 visits: an element of it)
    assert same(host(res.contribution), np.median(cf[inverse], axis=0))
    # the store equals the rows of eval_params over the five samples in one chunk (the seams)
    pressure = np.asarray(atm.pressure, float)
    out = torch.full((5, L, nb), float('nan'), dtype=torch.float64, device='cuda')
    model.eval_params(atm, unique, pb, chunk=5, contribution_out=out,
                      contribution_pressure=pressure, **kw)
    assert same(host(store), host(out.permute(1, 2, 0)))
    # the decks are seen: with every deck below the bottom of the grid the numbers are others
    deep = torch.empty_like(out)
    model.eval_params(atm, unique, pb, chunk=5, contribution_out=deep,
                      contribution_pressure=pressure,
                      **dict(kw, deck_logp=torch.full_like(kw['deck_logp'], 5.0)))
    assert not same(host(deep), host(out))
    # the other four products do not change
    plain = model.posterior_summary(atm, unique, counts, pb, chunk=CHUNK, keep_stores=True, **kw)
    assert plain.contribution is None and 'contribution' not in plain.stores
    for name in ('spectrum', 'bands', 'temperature', 'vmr'):
        assert torch.equal(getattr(plain, name), getattr(res, name)), name
    # one sample outside the table's temperatures: count 0, the median of the other four
    bad = chain[u_index].copy()
    bad[2, 4] = hot
    rej = model.posterior_summary(atm, eng.dev(bad), counts, pb, chunk=CHUNK, keep_stores=True,
                                  contribution=True, **kw)
    assert rej.n_rejected == 1
    keep = np.array([0, 1, 3, 4])
    cf = np.moveaxis(host(rej.stores['contribution']), -1, 0)
    full = cf[keep][np.repeat(np.arange(4), counts[keep])]
    if len(full) % 2:
        assert same(host(rej.contribution), np.median(full, axis=0))
    else:
        # (an even chain: np.median takes the mean of the two middle elements, the 0.5 quantile
        # np.percentile's lerp between them -- one rounding apart)
        assert same(host(rej.contribution), np.percentile(full, 50, axis=0))
        np.testing.assert_allclose(host(rej.contribution), np.median(full, axis=0), rtol=4e-16,
                                   atol=0)
