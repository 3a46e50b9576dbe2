"""posterior_summary(..., contribution=True): the reference's fifth product, the median of the band
contribution functions over the chain (tools/retrieval_tools.py:474-504:
np.median(cf[uinv], axis=0)), on the small chains of test_gpu_posterior.py -- five unique samples
with counts [3, 1, 4, 1, 2] (11 visits: the median is an element of the expansion) in chunks of 2,
and one sample the batch rejects.  Everything is for equal bits, as for the other four products."""
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


@pytest.mark.parametrize('geometry', ['transit', 'emission', 'two_stream'])
def test_posterior_contribution(eng, pa, g7, geometry):
    import torch
    model, atm, params, pb, kw, hot = tpost.atmosphere_case(eng, pa, g7, geometry)
    chain = np.repeat(params, COUNTS, axis=0)[np.random.default_rng(1).permutation(COUNTS.sum())]
    u_index, counts, inverse = post.unique_samples(chain)
    unique = eng.dev(chain[u_index])
    L, nb = model.nlayers, pb.nbands
    res = model.posterior_summary(atm, unique, counts, pb, chunk=CHUNK, keep_stores=True,
                                  contribution=True, **kw)
    assert res.contribution.shape == (L, nb)
    store = res.stores['contribution']
    assert store.shape == (L, nb, 5)
    cf = np.moveaxis(host(store), -1, 0)                       # [n, L, nbands]
    finite = np.isfinite(cf).all(axis=(0, 1))
    assert finite.any()                                        # (not every band has one sample)
    assert np.all(cf[:, :, finite].max(axis=1) == 1.0)
    assert same(host(res.contribution), np.median(cf[inverse], axis=0))
    # the store: one call over the five samples (the chunks' seams)
    prof = atm.evaluate(unique)
    ckw = dict(kw)
    if prof.continuum_density is not None:
        ckw.update(continuum_density=prof.continuum_density, alkali_density=prof.alkali_density)
    out = torch.empty((5, L, nb), dtype=torch.float64, device='cuda')
    model.eval_bands(prof.temps, prof.dens, pb, radius=prof.radius, chunk=5, contribution_out=out,
                     contribution_pressure=np.asarray(atm.pressure, float), **ckw)
    assert same(host(store), host(out.permute(1, 2, 0)))
    # eval_params passes both keywords through
    out2 = torch.empty_like(out)
    model.eval_params(atm, unique, pb, chunk=5, contribution_out=out2,
                      contribution_pressure=np.asarray(atm.pressure, float), **kw)
    assert same(host(out2), host(out))
    # the other four products do not change, and without the keyword the field is None
    plain = model.posterior_summary(atm, unique, counts, pb, chunk=CHUNK, keep_stores=True, **kw)
    assert plain.contribution is None and 'contribution' not in plain.stores
    for name in ('spectrum', 'bands', 'temperature', 'vmr'):
        assert torch.equal(getattr(plain, name), getattr(res, name)), name
    assert model.posterior_summary(atm, unique, counts, pb, contribution=True,
                                   **kw).stores is None
    # one sample outside the table's temperatures: count 0, the median of the other four
    bad = chain[u_index].copy()
    bad[2, 0 if geometry == 'two_stream' else 4] = hot
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


def test_contribution_arguments(eng, pa, g7):
    model, atm, params, pb, kw, hot = tpost.atmosphere_case(eng, pa, g7, 'transit')
    unique = eng.dev(params)
    for name in ('contribution_out', 'contribution_pressure'):
        with pytest.raises(ValueError, match=name):
            model.posterior_summary(atm, unique, COUNTS, pb, **{name: None})
