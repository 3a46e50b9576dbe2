"""Nested sampling on the device (csrc/pb_nested.hip, pyratbay_amd/nested.py) against its NumPy
statements, at the C ABI on NaN-filled outputs with a guard row behind them:

  * pb_nested_select against select_host: the order exact (ties, -inf, -1e98, NaN), the dead rows
    in bits, ln X, ln w, ln Z to 1e-13;
  * pb_nested_propose against start_host / propose_host: starts, a, b, gamma, inside exact, the
    points in bits;
  * pb_nested_accept against accept_host over 30 successive steps;
  * pb_nested_finish and pb_nested_resample against finish_host and resample_host;
  * every refusal;
  * NestedSampler on the Gaussian target of nested_cases against run_host, a run in two parts,
    the read-backs, and the committed bounds of the evidence;
  * Retrieval.nested / summary on test_gpu_retrieval's small emission model."""
import numpy as np
import pytest

import nested_cases as nc
import sampler_cases as sc
from test_gpu_sampler import no_read_back

pytestmark = pytest.mark.gpu

SEED = 0x1234567887654321


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def nan_tensor(shape):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')


def int_tensor(shape, kind='int32', value=-77):
    import torch
    return torch.full(shape, value, dtype=getattr(torch, kind), device='cuda')


def i32(eng, a):
    import torch
    return eng.dev(np.asarray(a), torch.int32)


def assert_close(got, want, rtol):
    """Finite values within rtol of each other; the others (-inf, +inf, NaN) the same."""
    got, want = np.atleast_1d(got).astype(float), np.atleast_1d(want).astype(float)
    finite = np.isfinite(want)
    assert np.array_equal(got[~finite], want[~finite], equal_nan=True), (got, want)
    assert np.all(np.abs(got[finite] - want[finite]) <= rtol * np.abs(want[finite])), \
        np.max(np.abs(got[finite] / want[finite] - 1))


# -------------------------------------------------------------------------------------------------
# pb_nested_select
# -------------------------------------------------------------------------------------------------
def run_select(eng, live_u, live_logl, ln_x, ln_z, K, dead_base=5):
    """pb_nested_select with dead_base rows already in the store and room for exactly K more."""
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    nlive, nfree = live_u.shape
    cap = dead_base + K
    dead_idx, surv_idx = int_tensor((K + 1,)), int_tensor((nlive - K + 1,))
    dead_u, dead_logl, dead_logw = nan_tensor((cap + 1, nfree)), nan_tensor((cap + 1,)), \
        nan_tensor((cap + 1,))
    state = eng.dev(np.array([ln_x, ln_z, 123.0, 456.0, 7.0]))
    u_d, l_d = eng.dev(live_u), eng.dev(live_logl)
    _capi.call('pb_nested_select', _ptr(dead_idx), _ptr(surv_idx), _ptr(dead_u), _ptr(dead_logl),
               _ptr(dead_logw), _ptr(state), _ptr(u_d), _ptr(l_d), dead_base, cap, K, nlive,
               nfree, _stream())
    torch.cuda.synchronize()
    assert int(dead_idx[K]) == -77 and int(surv_idx[nlive - K]) == -77 and float(state[4]) == 7.0
    for t in (dead_u, dead_logl, dead_logw):
        assert bool(torch.isnan(t[:dead_base]).all()) and bool(torch.isnan(t[cap]).all())
    assert np.array_equal(bits(host(u_d)), bits(live_u))
    return (host(dead_idx[:K]), host(surv_idx[:nlive - K]), host(dead_u[dead_base:cap]),
            host(dead_logl[dead_base:cap]), host(dead_logw[dead_base:cap]), host(state[:4]))


def check_select(eng, live_u, live_logl, ln_x, ln_z, K):
    from pyratbay_amd import nested
    want = nested.select_host(live_logl, ln_x, ln_z, K)
    dead_idx, surv_idx, dead_u, dead_logl, dead_logw, state = run_select(
        eng, live_u, live_logl, ln_x, ln_z, K)
    assert np.array_equal(dead_idx, want.dead_idx), (dead_idx, want.dead_idx)
    assert np.array_equal(surv_idx, want.surv_idx)
    assert np.array_equal(bits(dead_u), bits(live_u[want.dead_idx]))
    assert np.array_equal(bits(dead_logl), bits(want.dead_logl))
    assert_close(dead_logw, want.dead_logw, 1e-13)
    assert_close(state[0], want.ln_x, 1e-13)
    assert_close(state[1], want.ln_z, 1e-13)
    assert bits(state[2]) == bits(want.lstar)
    # remain is a difference of two values of the size of ln Z, each good to 1e-13
    if np.isfinite(want.remain):
        assert abs(state[3] - want.remain) <= 4e-13 * max(abs(want.ln_z), abs(want.remain), 1.0)
    else:
        assert_close(state[3], want.remain, 0.0)
    return want


@pytest.mark.parametrize('nlive', nc.NLIVES)
def test_select_against_the_host_statement(eng, nlive):
    rng = np.random.default_rng(nlive)
    nfree = {3: 1, 65: 128}.get(nlive, 3)
    live_u = rng.uniform(0, 1, (nlive, nfree))
    live_logl = nc.select_logl(nlive, nlive)
    for K in nc.batches(nlive):
        want = check_select(eng, live_u, live_logl, -0.75, -31.0, K)
        if nlive >= 5:
            assert np.isnan(want.dead_logl[0])
    # the first iteration: ln Z from -inf (and, where the first to die weigh nothing, still there)
    check_select(eng, live_u, live_logl, 0.0, -np.inf, 1)


def test_select_special_values(eng):
    logl = nc.special_logl()
    live_u = np.random.default_rng(1).uniform(0, 1, (len(logl), 2))
    for K in (1, 2, 3, 5, 10):
        want = check_select(eng, live_u, logl, 0.0, -np.inf, K)
        assert list(want.dead_idx) == [3, 5, 11, 1, 8, 2, 7, 0, 4, 9][:K]
    # every point the same; every point a NaN
    for value in (-4.0, np.nan):
        want = check_select(eng, live_u, np.full(len(logl), value), -1.0, -20.0, 4)
        assert list(want.dead_idx) == [0, 1, 2, 3]


# -------------------------------------------------------------------------------------------------
# pb_nested_propose
# -------------------------------------------------------------------------------------------------
def run_propose(eng, c):
    """One call of nc.propose_expectations on the device -> a dict of what it wrote."""
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    K, nfree = c['cur'].shape
    point = nan_tensor((K + 1, nfree))
    inside, a, b = int_tensor((K + 1,)), int_tensor((K + 1,)), int_tensor((K + 1,))
    gamma = nan_tensor((K + 1,))
    cur, cur_logl = nan_tensor((K + 1, nfree)), nan_tensor((K + 1,))
    acc_it = int_tensor((K + 1,))
    if not c['start']:
        cur[:K] = eng.dev(c['cur'])
        cur_logl[:K] = eng.dev(c['cur_logl'])
    live_u, live_logl, surv = eng.dev(c['live_u']), eng.dev(c['live_logl']), \
        i32(eng, c['surv_idx'])
    _capi.call('pb_nested_propose', _ptr(point), _ptr(inside), _ptr(a), _ptr(b), _ptr(gamma),
               _ptr(cur), _ptr(cur_logl), _ptr(acc_it), _ptr(live_u), _ptr(live_logl), _ptr(surv),
               c['it'], c['q'], c['seed'], nc.FGAMMA, nc.P_UNIT, int(c['start']), c['nlive'],
               nfree, K, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(point[K]).all()) and bool(torch.isnan(cur[K]).all())
    assert bool(torch.isnan(gamma[K])) and bool(torch.isnan(cur_logl[K]))
    for t in (inside, a, b, acc_it):
        assert int(t[K]) == -77
    assert np.array_equal(bits(host(live_u)), bits(c['live_u']))
    return dict(point=host(point[:K]), inside=host(inside[:K]), a=host(a[:K]), b=host(b[:K]),
                gamma=host(gamma[:K]), cur=host(cur[:K]), cur_logl=host(cur_logl[:K]),
                acc_it=host(acc_it[:K]))


@pytest.mark.parametrize('K', nc.KS)
@pytest.mark.parametrize('nfree', nc.NFREES)
def test_propose_against_the_host_statement(eng, nfree, K):
    seen = set()
    for c in nc.propose_expectations(nfree, K, SEED):
        got = run_propose(eng, c)
        # the starts (or the slots as they were), then the draw, then the points
        assert np.array_equal(bits(got['cur']), bits(c['cur']))
        assert np.array_equal(bits(got['cur_logl']), bits(c['cur_logl']))
        assert np.all(got['acc_it'] == (0 if c['start'] else -77))
        assert np.array_equal(got['a'], c['a']) and np.array_equal(got['b'], c['b'])
        assert np.array_equal(bits(got['gamma']), bits(c['gamma']))
        assert np.array_equal(got['inside'], c['inside'])
        assert np.array_equal(bits(got['point']), bits(c['point']))
        ins = c['inside'] == 1
        assert np.array_equal(bits(got['point'][ins]), bits(c['prop'][ins]))
        assert np.array_equal(bits(got['point'][~ins]), bits(c['cur'][~ins]))
        seen |= set(got['inside'])
    assert seen == {0, 1}


# -------------------------------------------------------------------------------------------------
# pb_nested_accept
# -------------------------------------------------------------------------------------------------
NSTEPS_ACCEPT = 30


@pytest.mark.parametrize('K', nc.KS)
@pytest.mark.parametrize('nfree', [1, 65, 128])
def test_accept_against_the_host_statement(eng, nfree, K):
    """30 successive steps in iterations of five: the decisions of every slot at every step, then
    the whole state."""
    import torch
    from pyratbay_amd import _capi, nested
    from pyratbay_amd._device import _ptr, _stream
    rng = np.random.default_rng(1000 * nfree + K)
    st = nc.accept_case(nfree, K, 1000 * nfree + K)
    nlive = st.live_u.shape[0]
    live0 = st.live_u.copy()
    cur, cur_logl = nan_tensor((K + 1, nfree)), nan_tensor((K + 1,))
    cur[:K], cur_logl[:K] = eng.dev(st.cur), eng.dev(st.cur_logl)
    live_u, live_logl = nan_tensor((nlive + 1, nfree)), nan_tensor((nlive + 1,))
    live_u[:nlive], live_logl[:nlive] = eng.dev(st.live_u), eng.dev(st.live_logl)
    naccept, stuck = int_tensor((K + 1,), 'int64', 0), int_tensor((K + 1,), 'int64', 0)
    acc_it = int_tensor((K + 1,), 'int32', 0)
    dead_idx = i32(eng, st.dead_idx)
    taken, special = 0, set()
    for step in range(NSTEPS_ACCEPT):
        if step % 5 == 0:
            lstar = float(rng.uniform(-12.0, -8.0))
            st.acc_it[:] = 0
            acc_it.zero_()
        last = step % 5 == 4
        point, logl_prop, inside = nc.accept_inputs(st, step, rng, lstar)
        special |= {repr(float(v)) for v in logl_prop if not np.isfinite(v)}
        accepted = int_tensor((K + 1,))
        state = eng.dev(np.array([np.nan, np.nan, lstar, np.nan]))
        point_d, logl_d, inside_d = eng.dev(point), eng.dev(logl_prop), i32(eng, inside)
        _capi.call('pb_nested_accept', _ptr(cur), _ptr(cur_logl), _ptr(point_d), _ptr(logl_d),
                   _ptr(inside_d), _ptr(state), _ptr(naccept), _ptr(acc_it), _ptr(stuck),
                   _ptr(accepted), _ptr(live_u), _ptr(live_logl), _ptr(dead_idx), int(last),
                   nlive, nfree, K, _stream())
        want = nested.accept_host(st, point, logl_prop, inside, lstar,
                                  st.dead_idx if last else None)
        got = host(accepted)
        assert got[K] == -77 and np.array_equal(got[:K], want), (step, got, want)
        with np.errstate(invalid='ignore'):
            never = np.isnan(logl_prop) | (logl_prop == -np.inf) | (inside == 0)
        assert not np.any(want[never])
        taken += int(want.sum())
        assert np.array_equal(bits(host(cur[:K])), bits(st.cur)), step
        assert np.array_equal(bits(host(live_u[:nlive])), bits(st.live_u)), step
    assert 0 < taken < NSTEPS_ACCEPT * K
    if K >= 3:
        assert special == {'nan', '-inf', 'inf'}
    assert np.array_equal(bits(host(cur_logl[:K])), bits(st.cur_logl))
    assert np.array_equal(bits(host(live_logl[:nlive])), bits(st.live_logl))
    assert np.array_equal(host(naccept[:K]), st.naccept) and st.naccept.sum() == taken
    assert np.array_equal(host(acc_it[:K]), st.acc_it)
    assert np.array_equal(host(stuck[:K]), st.stuck)
    if K >= 65:
        assert st.stuck.sum() > 0
    # the guards, and the rows of the survivors
    assert bool(torch.isnan(cur[K]).all()) and bool(torch.isnan(live_u[nlive]).all())
    assert bool(torch.isnan(cur_logl[K])) and bool(torch.isnan(live_logl[nlive]))
    assert int(naccept[K]) == 0 and int(stuck[K]) == 0 and int(acc_it[K]) == 0
    others = np.setdiff1d(np.arange(nlive), st.dead_idx)
    assert np.array_equal(bits(host(live_u)[others]), bits(live0[others]))


# -------------------------------------------------------------------------------------------------
# pb_nested_finish, pb_nested_resample
# -------------------------------------------------------------------------------------------------
def run_finish(eng, dead_logl, dead_logw, live_logl, ln_x):
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    ndead, nlive = len(dead_logl), len(live_logl)
    n = ndead + nlive
    out = nan_tensor((4,))
    logw, logl, cdf = nan_tensor((n + 1,)), nan_tensor((n + 1,)), nan_tensor((n + 1,))
    state = eng.dev(np.array([ln_x, np.nan, np.nan, np.nan]))
    # (two more rows in the store than the run has written)
    dl = eng.dev(np.concatenate((dead_logl, [1e300, np.nan])))
    dw = eng.dev(np.concatenate((dead_logw, [1e300, np.nan])))
    ll = eng.dev(live_logl)
    _capi.call('pb_nested_finish', _ptr(out), _ptr(logw), _ptr(logl), _ptr(cdf), _ptr(dl),
               _ptr(dw), _ptr(ll), _ptr(state), ndead, nlive, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[3])) and bool(torch.isnan(logw[n])) and \
        bool(torch.isnan(logl[n])) and bool(torch.isnan(cdf[n]))
    return host(out[:3]), host(logw[:n]), host(logl[:n]), cdf[:n]


def run_resample(cdf_d, nsamples, seed):
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    n = cdf_d.shape[0]
    counts = int_tensor((n + 1,), 'int64')
    _capi.call('pb_nested_resample', _ptr(counts), _ptr(cdf_d), n, nsamples, seed, _stream())
    torch.cuda.synchronize()
    assert int(counts[n]) == -77
    return host(counts[:n])


@pytest.mark.parametrize('ndead,nlive', nc.FINISH_SHAPES)
def test_finish_and_resample(eng, ndead, nlive):
    from pyratbay_amd import nested
    dead_logl, dead_logw, live_logl, ln_x = nc.finish_case(ndead, nlive, ndead + nlive)
    want = nested.finish_host(dead_logl, dead_logw, live_logl, ln_x)
    out, logw, logl, cdf_d = run_finish(eng, dead_logl, dead_logw, live_logl, ln_x)
    cdf = host(cdf_d)
    assert np.array_equal(bits(logl), bits(want.logl))
    assert_close(logw, want.logw, 1e-15)
    assert_close(out, [want.ln_z, want.ln_z_err, want.info], 1e-12)
    assert np.all(np.diff(cdf) >= 0) and np.all(np.abs(cdf - want.cdf) <= 1e-13)
    n = ndead + nlive
    for nsamples in nc.resample_counts(n):
        # the host's cdf on the device: the same bits in, the same counts out
        assert np.array_equal(run_resample(eng.dev(want.cdf), nsamples, SEED + nsamples),
                              nested.resample_host(want.cdf, nsamples, SEED + nsamples))
        # the device's cdf: the draws that come within 1e-12 of a cdf value may fall either way
        got = run_resample(cdf_d, nsamples, SEED + nsamples)
        assert got.sum() == nsamples and not got[want.logw == -np.inf].any()
        u = nested.resample_uniforms_host(SEED + nsamples, nsamples)
        index, near = nc.near_cdf(want.cdf, u)
        assert near.mean() <= 0.01              # (test_nested_cpu: it holds on the host alone)
        clear = np.bincount(index[~near], minlength=n)
        assert np.all(got >= clear) and (got - clear).sum() == near.sum()
    assert np.array_equal(run_resample(cdf_d, 0, 1), np.zeros(n, np.int64))


# -------------------------------------------------------------------------------------------------
# refusals
# -------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    PbError = _capi.PbError
    f = nan_tensor((4200 * 3,))
    i = int_tensor((4200,), 'int64', 0)
    p, q, s = _ptr(f), _ptr(i), _stream()

    def select(*tail, ptrs=None):
        _capi.call('pb_nested_select', *(ptrs or [q, q, p, p, p, p, p, p]), *tail, s)

    def propose(*tail, ptrs=None):
        _capi.call('pb_nested_propose', *(ptrs or [p, q, q, q, p, p, p, q, p, p, q]), *tail, s)

    def accept(*tail, ptrs=None):
        _capi.call('pb_nested_accept', *(ptrs or [p, p, p, p, q, p, q, q, q, q, p, p, q]), *tail,
                   s)
    # (dead_base, dead_cap, K, nlive, nfree)
    for K, nlive in ((0, 10), (9, 10), (-1, 10), (1, 2)):
        with pytest.raises(PbError, match=f'pb_nested_select: a batch of {K} with {nlive} live '
                                          'points: 1 <= batch <= nlive - 2'):
            select(0, 100, K, nlive, 3)
    with pytest.raises(PbError, match='pb_nested_select: 4097 live points: at most 4096'):
        select(0, 5000, 4, 4097, 3)
    with pytest.raises(PbError, match='pb_nested_select: 129 free parameters: at most 128'):
        select(0, 100, 4, 10, 129)
    with pytest.raises(PbError, match='pb_nested_select: 4 rows behind 98 dead points: the store '
                                      'holds 100'):
        select(98, 100, 4, 10, 3)
    for k in range(8):
        ptrs = [q, q, p, p, p, p, p, p]
        ptrs[k] = None
        with pytest.raises(PbError, match='pb_nested_select: null pointer'):
            select(0, 100, 4, 10, 3, ptrs=ptrs)
    # (it, q, seed, fgamma, p_unit, start, nlive, nfree, K)
    with pytest.raises(PbError, match='pb_nested_propose: a batch of 9 with 10 live points'):
        propose(1, 0, 0, 1.0, 0.1, 1, 10, 3, 9)
    with pytest.raises(PbError, match='pb_nested_propose: 4097 live points: at most 4096'):
        propose(1, 0, 0, 1.0, 0.1, 1, 4097, 3, 4)
    with pytest.raises(PbError, match='pb_nested_propose: 129 free parameters: at most 128'):
        propose(1, 0, 0, 1.0, 0.1, 1, 10, 129, 4)
    with pytest.raises(PbError, match=r'iteration 4294967296: the counter holds 0 <= it < 2\^32'):
        propose(2**32, 0, 0, 1.0, 0.1, 1, 10, 3, 4)
    with pytest.raises(PbError, match=r'step 4294967296: the counter holds 0 <= q < 2\^32'):
        propose(1, 2**32, 0, 1.0, 0.1, 1, 10, 3, 4)
    with pytest.raises(PbError, match=r'step -1: the counter holds'):
        propose(1, -1, 0, 1.0, 0.1, 1, 10, 3, 4)
    for k in range(11):
        ptrs = [p, q, q, q, p, p, p, q, p, p, q]
        ptrs[k] = None
        with pytest.raises(PbError, match='pb_nested_propose: null pointer'):
            propose(1, 0, 0, 1.0, 0.1, 1, 10, 3, 4, ptrs=ptrs)
    # (last, nlive, nfree, K)
    with pytest.raises(PbError, match='pb_nested_accept: a batch of 9 with 10 live points'):
        accept(1, 10, 3, 9)
    with pytest.raises(PbError, match='pb_nested_accept: 4097 live points: at most 4096'):
        accept(1, 4097, 3, 4)
    with pytest.raises(PbError, match='pb_nested_accept: 129 free parameters: at most 128'):
        accept(1, 10, 129, 4)
    for k in range(13):
        ptrs = [p, p, p, p, q, p, q, q, q, q, p, p, q]
        ptrs[k] = None
        with pytest.raises(PbError, match='pb_nested_accept: null pointer'):
            accept(1, 10, 3, 4, ptrs=ptrs)
    # no slots: nothing launched, whatever the pointers
    propose(1, 0, 0, 1.0, 0.1, 1, 10, 3, 0, ptrs=[None] * 11)
    accept(1, 10, 3, 0, ptrs=[None] * 13)
    # finish(out, logw, logl, cdf, dead_logl, dead_logw, live_logl, state, ndead, nlive)
    with pytest.raises(PbError, match='pb_nested_finish: null pointer'):
        _capi.call('pb_nested_finish', p, p, p, p, None, p, p, p, 5, 4, s)
    with pytest.raises(PbError, match='pb_nested_finish: null pointer'):
        _capi.call('pb_nested_finish', None, p, p, p, p, p, p, p, 5, 4, s)
    with pytest.raises(PbError, match='pb_nested_finish: 4097 live points: at most 4096'):
        _capi.call('pb_nested_finish', p, p, p, p, p, p, p, p, 5, 4097, s)
    with pytest.raises(PbError, match='pb_nested_finish: bad shape'):
        _capi.call('pb_nested_finish', p, p, p, p, p, p, p, p, -1, 4, s)
    with pytest.raises(PbError, match='pb_nested_resample: null pointer'):
        _capi.call('pb_nested_resample', q, None, 5, 5, 0, s)
    with pytest.raises(PbError, match=r'pb_nested_resample: 4294967297 samples: at most 2\^32'):
        _capi.call('pb_nested_resample', q, p, 5, 2**32 + 1, 0, s)
    with pytest.raises(PbError, match='pb_nested_resample: bad shape'):
        _capi.call('pb_nested_resample', q, p, 0, 5, 0, s)


# -------------------------------------------------------------------------------------------------
# the loop on the device against the loop on the host
# -------------------------------------------------------------------------------------------------
SMALL = dict(nlive=64, batch=16, nsteps=8)


def gaussian_sampler(eng, seed=0, **kw):
    log_like, prior_transform = nc.target_torch()
    kw = kw or SMALL
    return eng.NestedSampler(log_like, prior_transform, 3, kw['nlive'], batch=kw['batch'],
                             nsteps=kw['nsteps'], seed=seed).start()


def test_device_loop_against_the_host_loop(eng):
    import torch
    want = nc.gaussian_run_host(0, 64, 16, 8, 15, None)
    margin = np.array(want.margin)
    assert np.all(np.abs(margin[np.isfinite(margin)]) > 1e-9)
    # (the replacement a stuck slot leaves is a copy of a survivor: an exact tie, by index)
    ranked = np.diff(np.sort(want.dead_logl))
    assert np.all(ranked[ranked > 0] > 1e-9)
    ns = gaussian_sampler(eng)
    ns.trace = []
    ns.run(15)
    assert ns.it == 15 and ns.ndead == 240
    assert np.array_equal(host(torch.stack([d for d, _ in ns.trace])), np.array(want.dead_idx))
    assert np.array_equal(host(torch.stack([a for _, a in ns.trace])), np.array(want.accepted))
    assert np.all(np.abs(host(ns.live_u) - want.live_u) <= 1e-10)
    assert np.all(np.abs(host(ns.live_logl) - want.live_logl) <= 1e-10)
    assert np.all(np.abs(host(ns.dead_u[:240]) - want.dead_u) <= 1e-10)
    assert np.all(np.abs(host(ns.dead_logl[:240]) - want.dead_logl) <= 1e-10)
    assert np.all(np.abs(host(ns.dead_logw[:240]) - want.dead_logw) <= 1e-10)
    np.testing.assert_allclose(host(ns.state), [want.ln_x, want.ln_z, want.lstar, want.remain],
                               rtol=1e-10)
    assert np.array_equal(host(ns.naccept), want.naccept)
    assert int(ns.stuck()) == want.stuck.sum()
    assert float(ns.efficiency()) == want.naccept.sum() / (15.0 * 8 * 16)
    # the result: finish_host on the host's run
    lnz, err, _, fin = nc.result_host(want, 0)
    np.testing.assert_allclose(host(ns.logz()), [lnz, err, fin.info], rtol=1e-9)
    theta, logw, logl = ns.weighted()
    assert theta.shape == (240 + 64, 3) and logw.shape == logl.shape == (304,)
    np.testing.assert_allclose(host(logw), fin.logw, rtol=1e-10)
    # finish disturbs nothing; one run of 15, launches only; 9 + 6: the same bits
    whole = gaussian_sampler(eng)
    assert no_read_back(lambda: whole.run(15)) == []
    parts = gaussian_sampler(eng).run(9)
    parts.logz(), parts.unique()
    parts.run(6)
    for name in ('live_u', 'live_logl', 'state', 'cur', 'cur_logl', 'naccept', 'stuck_slots',
                 'dead_idx', 'surv_idx'):
        assert torch.equal(getattr(parts, name), getattr(whole, name)), name
        assert torch.equal(getattr(ns, name), getattr(whole, name)), name
    for name in ('dead_u', 'dead_logl', 'dead_logw'):
        assert torch.equal(getattr(parts, name)[:240], getattr(whole, name)[:240]), name
    # the dead store doubles: a run beyond its first 16 batches keeps what it had
    more = gaussian_sampler(eng).run(20)
    assert more.dead_cap >= 320 and torch.equal(more.dead_u[:240], whole.dead_u[:240])
    # run_until: one double per look
    looks = gaussian_sampler(eng)
    assert no_read_back(lambda: looks.run_until(1e-300, check_every=3, max_iter=9)) == ['item'] * 3
    assert looks.it == 9
    assert no_read_back(lambda: looks.run_until(1e300, check_every=4, max_iter=40)) == ['item']
    assert looks.it == 13
    # unique: the form posterior_summary takes
    theta, counts = whole.unique()
    assert counts.dtype == torch.int64 and int(counts.sum()) == 304 and bool((counts > 0).all())
    assert theta.shape == (counts.shape[0], 3)
    theta, counts = whole.unique(nsamples=5000)
    assert int(counts.sum()) == 5000
    with pytest.raises(ValueError, match='no burn-in'):
        whole.unique(burn=3)
    with pytest.raises(ValueError, match='log_like must return a float64 device tensor'):
        eng.NestedSampler(lambda t: t[:, 0].float(), lambda c: c, 3, 64).start()


def test_device_loop_finds_the_evidence(eng):
    """nlive 512, batch 128, nsteps 30, dlogz 0.01 at seed 0 on the device: the bounds committed
    for the host statement."""
    ns = gaussian_sampler(eng, nlive=nc.NLIVE, batch=nc.BATCH, nsteps=nc.NSTEPS)
    ns.run_until(nc.DLOGZ, check_every=1, max_iter=nc.MAX_ITER)
    lnz, err, info = host(ns.logz())
    theta, counts = ns.unique()
    mean, std, corr = sc.statistics(host(theta), host(counts).astype(float))
    print(f'{ns.it} iterations, ln Z {lnz:.4f} +- {err:.4f} against {nc.LN_Z:.4f}, H {info:.3f}, '
          f'efficiency {float(ns.efficiency()):.3f}, stuck {int(ns.stuck())}; worst |mean - mu| '
          f'/ sigma {mean:.4f}, relative error of sigma {std:.4f}, correlation error {corr:.4f}')
    assert ns.it < nc.MAX_ITER and float(ns.state[3]) < nc.DLOGZ
    assert abs(lnz - nc.LN_Z) <= nc.BOUND_LNZ
    assert mean <= nc.BOUND_MEAN and std <= nc.BOUND_STD and corr <= nc.BOUND_CORR
    assert 0.2 < float(ns.efficiency()) < 0.5


# -------------------------------------------------------------------------------------------------
# Retrieval.nested / summary
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def retrieval(eng, golden):
    return sc.emission_retrieval(eng, golden)


def test_retrieval_nested_end_to_end(eng, retrieval):
    """32 live points, batches of 8, 4 steps, 6 iterations against run_host over the device's
    log_likelihood and prior_transform."""
    import torch
    from pyratbay_amd import nested
    ret = retrieval
    ns = ret.nested(nlive=32, seed=5, dlogz=None, batch=8, nsteps=4)
    assert ns.it == 0 and ns.nfree == ret.nfree
    ns.trace = []
    ns.run(6)

    def log_like(theta):
        return host(ret.log_likelihood(eng.dev(theta)))

    def prior_transform(cube):
        return host(ret.prior_transform(eng.dev(cube)))
    want = nested.run_host(log_like, prior_transform, 32, 8, 4, 6, seed=5, nfree=ret.nfree)
    # margins: none within 1e-9 of the threshold, but for exact ties at the reject value (draws
    # from the prior that the model refuses): -1e98 against a threshold of -1e98 rejects
    margin = np.array(want.margin)
    lstar = want.dead_logl.reshape(6, 8)[:, -1]
    tie = (margin == 0.0) & (lstar == -1e98)[:, None, None]
    assert np.all(np.abs(margin[np.isfinite(margin) & ~tie]) > 1e-9)
    assert np.array_equal(host(torch.stack([d for d, _ in ns.trace])), np.array(want.dead_idx))
    assert np.array_equal(host(torch.stack([a for _, a in ns.trace])), np.array(want.accepted))
    assert 0 < want.naccept.sum() < 6 * 4 * 8
    assert np.all(np.abs(host(ns.live_u) - want.live_u) <= 1e-10)
    assert np.all(np.abs(host(ns.dead_u[:48]) - want.dead_u) <= 1e-10)
    lnz = host(ns.logz())
    assert np.all(np.isfinite(lnz)) and lnz[1] > 0
    theta, counts = ns.unique()
    assert int(counts.sum()) == 48 + 32 and theta.shape[1] == ret.nfree
    summary = ret.summary(ns)
    assert int(summary.n_rejected) == 0
    assert bool(torch.isfinite(summary.bands[0]).all())
    # the whole front door: started and run until the evidence to come is small
    done = ret.nested(nlive=32, seed=5, dlogz=1e300, batch=8, nsteps=4, check_every=2)
    assert done.it == 2
    # a uniform parameter with an infinite bound is refused before anything is launched
    calls = []
    real = ret.log_likelihood
    ret.log_likelihood = lambda t: (calls.append(t.shape[0]), real(t))[1]
    k = ret.ifree[0]
    pmax = ret.pmax[k]
    ret.pmax[k] = np.inf
    try:
        with pytest.raises(ValueError, match='have an infinite bound'):
            ret.nested(nlive=32, seed=5)
    finally:
        ret.pmax[k] = pmax
        del ret.log_likelihood
    assert calls == []
