"""The sampler on the device (csrc/pb_sampler.hip, pyratbay_amd/sampler.py) against its NumPy
statements, at the C ABI on NaN-filled outputs:

  * pb_demc_propose against propose_host: kinds exact, parallel proposals without epsilon in bits
    (so r1, r2 are the host's), proposals and log_jac within PROPOSE_UNITS / LOGJAC_UNITS;
  * pb_demc_accept against accept_host over 50 successive calls: decisions, store, history, state
    exact, Welford's sums to 1e-13;
  * pb_gelman_rubin, pb_philox_uniform;
  * DEMC on the Gaussian target of sampler_cases against run_host: accept pattern, states, a run
    in two parts, unique, and the committed statistical bounds at 3000 generations;
  * Retrieval.sample / draw_initial / summary on test_gpu_retrieval's small emission model.

Measured on the device (profiles/sampler.md): the largest error of a proposal is 2.704 units of
eps times the scale below, of log_jac 0.854 units; each bound is the next power of two above four
times that.  Far above them the wrong thing is being computed; that is not a tolerance to widen."""
import numpy as np
import pytest

import sampler_cases as sc

pytestmark = pytest.mark.gpu

EPS = sc.EPS
PROPOSE_UNITS = 16.0
LOGJAC_UNITS = 4.0
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


# -------------------------------------------------------------------------------------------------
# pb_demc_propose
# -------------------------------------------------------------------------------------------------
def run_propose(eng, theta, z, M, pstep, g, seed, fgamma, fepsilon, p_snooker):
    """pb_demc_propose on NaN-filled outputs with a guard row behind them -> prop, log_jac, kind."""
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    nw, nfree = theta.shape
    prop = nan_tensor((nw + 1, nfree))
    log_jac = nan_tensor((nw + 1,))
    kind = torch.full((nw + 1,), -77, dtype=torch.int32, device='cuda')
    theta_d, z_d, pstep_d = eng.dev(theta), eng.dev(z), eng.dev(pstep)
    _capi.call('pb_demc_propose', _ptr(prop), _ptr(log_jac), _ptr(kind), _ptr(theta_d),
               _ptr(z_d), _ptr(pstep_d), g, seed, M, fgamma, fepsilon, p_snooker, nfree, nw,
               _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(prop[nw]).all()) and bool(torch.isnan(log_jac[nw]))
    assert int(kind[nw]) == -77
    return host(prop[:nw]), host(log_jac[:nw]), host(kind[:nw])


def snooker_terms(theta, z, d):
    """The quantities the snooker's bounds are made of, from the host's draw d (details of
    propose_host): cancellation of the dot product, the distance ratio, and per element the
    error scales of prop and of log_jac (module docstring of the scale: below)."""
    diff, zr = z[d.r1] - z[d.r2], z[d.rz]
    dd = theta - zr
    D2 = np.sum(dd * dd, axis=1)
    proj = np.sum(diff * dd, axis=1)
    cancel = np.sum(np.abs(diff * dd), axis=1) / np.abs(proj)
    ratio = np.sqrt(D2 / np.sum(theta * theta, axis=1))
    c = (1.2 + d.u_g) * (proj / D2)
    mag = np.abs(theta) + np.abs(zr)
    # prop = theta + c d: the rounding of theta + ., of d, and the relative error of c, which is
    # that of the two sums: the dot product's grows with its cancellation
    prop_scale = np.abs(theta) + (np.abs(c) * cancel)[:, None] * mag
    e = (theta + c[:, None] * dd) - zr
    N2 = np.sum(e * e, axis=1)
    # log_jac = 0.5 (nfree - 1) (ln N2 - ln D2): the logarithms' own rounding, and the relative
    # errors of N2 and D2 from their elements' errors
    amp_n = 2.0 * np.sum(np.abs(e) * (prop_scale + np.abs(zr)), axis=1) / N2
    amp_d = 2.0 * np.sum(np.abs(dd) * mag, axis=1) / D2
    nfree = theta.shape[1]
    lj_scale = 0.5 * (nfree - 1) * (np.abs(np.log(N2)) + np.abs(np.log(D2)) + amp_n + amp_d)
    return cancel, ratio, prop_scale, lj_scale


def propose_generations(theta, z, M, pstep, g0, count):
    """The first `count` generations from g0 on whose snooker proposals (host draw) all keep
    |theta - Z[rz]| >= 0.1 |theta| and the cancellation of the dot product <= 100."""
    from pyratbay_amd import sampler
    found = []
    for g in range(g0, g0 + 2000):
        *_, kind, d = sampler.propose_host(theta, z, M, pstep, g, SEED, sc.FGAMMA, sc.FEPSILON,
                                           sc.P_SNOOKER, details=True)
        snk = kind == 1
        with np.errstate(all='ignore'):
            cancel, ratio, _, _ = snooker_terms(theta, z, d)
        if np.all(ratio[snk] >= 0.1) and np.all(cancel[snk] <= 100.0):
            found.append(g)
            if len(found) == count:
                return found
    raise AssertionError('no generation with well-conditioned snooker proposals')


WORST = {'prop': 0.0, 'log_jac': 0.0}


@pytest.mark.parametrize('nw', sc.NWS)
@pytest.mark.parametrize('nfree', sc.NFREES)
def test_propose_against_the_host_statement(eng, nfree, nw):
    from pyratbay_amd import sampler
    gamma = sampler.gamma_host(sc.FGAMMA, nfree)
    for M in sc.MS:
        theta, z, pstep, g0 = sc.propose_case(nfree, nw, M, 7 * nfree + 100 * nw + M)
        kinds = []
        for g in propose_generations(theta, z, M, pstep, g0, {1: 12, 5: 4, 65: 2}[nw]):
            want, want_lj, want_kind, d = sampler.propose_host(
                theta, z, M, pstep, g, SEED, sc.FGAMMA, sc.FEPSILON, sc.P_SNOOKER, details=True)
            got, got_lj, got_kind = run_propose(eng, theta, z, M, pstep, g, SEED, sc.FGAMMA,
                                                sc.FEPSILON, sc.P_SNOOKER)
            assert np.array_equal(got_kind, want_kind)
            kinds += list(want_kind)
            par, snk = want_kind == 0, want_kind == 1
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(got_lj))
            # without epsilon a parallel proposal has the host's bits: the same r1 and r2
            plain = run_propose(eng, theta, z, M, pstep, g, SEED, sc.FGAMMA, 0.0, sc.P_SNOOKER)
            jump = theta + gamma * (z[d.r1] - z[d.r2])
            assert np.array_equal(bits(plain[0][par]), bits(jump[par]))
            assert np.array_equal(bits(plain[0][snk]), bits(got[snk]))
            assert np.array_equal(plain[2], want_kind)
            # parallel: theta + gamma (z1 - z2) + fepsilon pstep n
            scale = (np.abs(theta) + gamma * (np.abs(z[d.r1]) + np.abs(z[d.r2])) +
                     sc.FEPSILON * pstep * (1 + np.abs(d.normals)))
            units = np.abs(got - want) / (EPS * scale)
            assert np.all(got_lj[par] == 0.0)
            worst = float(np.max(units[par])) if par.any() else 0.0
            if snk.any():
                cancel, ratio, prop_scale, lj_scale = snooker_terms(theta, z, d)
                assert np.all(ratio[snk] >= 0.1) and np.all(cancel[snk] <= 100.0)
                units = np.abs(got - want) / (EPS * prop_scale)
                worst = max(worst, float(np.max(units[snk])))
                if nfree == 1:
                    assert np.all(got_lj == 0.0) and np.all(want_lj == 0.0)
                else:
                    lj_units = np.abs(got_lj - want_lj)[snk] / (EPS * lj_scale[snk])
                    WORST['log_jac'] = max(WORST['log_jac'], float(np.max(lj_units)))
                    assert np.max(lj_units) <= LOGJAC_UNITS
            WORST['prop'] = max(WORST['prop'], worst)
            assert worst <= PROPOSE_UNITS
        assert set(kinds) == {0, 1}
    print(f'propose nfree {nfree} nw {nw}: largest errors so far {WORST["prop"]:.3f} units '
          f'(prop), {WORST["log_jac"]:.3f} units (log_jac)')


def test_propose_degenerate_history_and_refusals(eng):
    from pyratbay_amd import _capi, sampler
    from pyratbay_amd._device import _ptr, _stream
    theta = np.tile(np.array([[0.3, -1.5, 2.0e3]]), (64, 1))
    z = np.tile(theta[:1], (5, 1))
    want, want_lj, want_kind = sampler.propose_host(theta, z, 5, np.ones(3), 7, 1, p_snooker=0.5)
    got, got_lj, got_kind = run_propose(eng, theta, z, 5, np.ones(3), 7, 1, 1.0, 0.0, 0.5)
    assert set(got_kind) == {0, 1} and np.array_equal(got_kind, want_kind)
    assert np.array_equal(bits(got), bits(theta)) and np.all(got_lj == 0.0)
    assert np.array_equal(bits(want), bits(theta)) and np.all(want_lj == 0.0)
    t = eng.dev(theta)
    args = [_ptr(t)] * 6
    with pytest.raises(_capi.PbError, match='a history of 2 rows: at least 3'):
        _capi.call('pb_demc_propose', *args, 1, 0, 2, 1.0, 0.0, 0.1, 3, 64, _stream())
    with pytest.raises(_capi.PbError, match='null pointer'):
        _capi.call('pb_demc_propose', *args[:5], None, 1, 0, 5, 1.0, 0.0, 0.1, 3, 64, _stream())
    with pytest.raises(_capi.PbError, match=r'generation 4294967296: the counter holds'):
        _capi.call('pb_demc_propose', *args, 2**32, 0, 5, 1.0, 0.0, 0.1, 3, 64, _stream())
    with pytest.raises(_capi.PbError, match='129 free parameters: at most 128'):
        _capi.call('pb_demc_propose', *args, 1, 0, 5, 1.0, 0.0, 0.1, 129, 64, _stream())
    # the last generation the counter holds is taken; no walkers: nothing launched
    _capi.call('pb_demc_propose', *args, 2**32 - 1, 0, 5, 1.0, 0.0, 0.1, 3, 1, _stream())
    _capi.call('pb_demc_propose', *([None] * 6), 1, 0, 5, 1.0, 0.0, 0.1, 3, 0, _stream())


# -------------------------------------------------------------------------------------------------
# pb_demc_accept
# -------------------------------------------------------------------------------------------------
STATE_F64 = ('theta', 'logp', 'rows', 'row_logp', 'mean', 'm2', 'z')
STATE_INT = {'row_gen': 'int32', 'counts': 'int64', 'nrows': 'int32', 'overflow': 'int32',
             'nstat': 'int64'}


def upload_state(eng, st):
    import torch
    d = {k: eng.dev(getattr(st, k)) for k in STATE_F64}
    d.update({k: eng.dev(getattr(st, k), getattr(torch, t)) for k, t in STATE_INT.items()})
    return d


def call_accept(eng, d, prop, logp_prop, log_jac, g, seed, M, Mcap, append, cap):
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    nw, nfree = prop.shape
    accepted = torch.full((nw + 1,), -77, dtype=torch.int32, device='cuda')
    prop_d, logp_prop_d, log_jac_d = eng.dev(prop), eng.dev(logp_prop), eng.dev(log_jac)
    _capi.call('pb_demc_accept', _ptr(d['theta']), _ptr(d['logp']), _ptr(prop_d),
               _ptr(logp_prop_d), _ptr(log_jac_d), _ptr(d['rows']),
               _ptr(d['row_logp']), _ptr(d['row_gen']), _ptr(d['counts']), _ptr(d['nrows']),
               _ptr(d['overflow']), _ptr(d['mean']), _ptr(d['m2']), _ptr(d['nstat']),
               _ptr(d['z']), _ptr(accepted), g, seed, M, Mcap, int(append), cap, nfree, nw,
               _stream())
    got = host(accepted)
    assert got[nw] == -77
    return got[:nw]


NCALLS = 50


@pytest.mark.parametrize('cap', [1, 4])
@pytest.mark.parametrize('nw', sc.NWS)
@pytest.mark.parametrize('nfree', [1, 65, 128])
def test_accept_against_the_host_statement(eng, nfree, nw, cap):
    """50 successive calls, every other one with append: the decisions of every walker at every
    call, then the whole state."""
    from pyratbay_amd import sampler
    seed = SEED + nfree
    rng = np.random.default_rng(1000 * nfree + 10 * nw + cap)
    st = sc.accept_case(nfree, nw, cap, 1000 * nfree + 10 * nw + cap)
    # room for the 25 appends and two guard rows behind them
    M0 = st.M
    st.Mcap = M0 + 25 * nw
    z = np.full((st.Mcap + 2, nfree), np.nan)
    z[:M0] = st.z[:M0]
    st.z = z
    d = upload_state(eng, st)
    states, taken, special = [], 0, set()
    g = 2**31 - 1 - NCALLS                              # (up to the last generation row_gen holds)
    for i in range(NCALLS):
        g += 1
        prop, logp_prop, log_jac = sc.accept_inputs(st, g, seed, rng)
        special |= {repr(float(v)) for v in logp_prop if not np.isfinite(v)}
        append = i % 2 == 1
        got = call_accept(eng, d, prop, logp_prop, log_jac, g, seed, st.M, st.Mcap, append, cap)
        want = sampler.accept_host(st, prop, logp_prop, log_jac, g, seed, append)
        assert np.array_equal(got, want), (i, got, want)
        # NaN and -inf reject, whatever the other terms
        with np.errstate(invalid='ignore'):
            dead = np.isnan(logp_prop) | np.isnan(log_jac) | (logp_prop == -np.inf)
        assert not np.any(want[dead])
        if append:
            st.M += nw
        taken += int(want.sum())
        states.append(st.theta.copy())
    assert st.M == st.Mcap and 0 < taken < NCALLS * nw
    if nw >= 5:
        assert special == {'nan', '-inf', 'inf'}
    assert np.any(st.overflow != 0) and np.all(st.nrows <= cap)
    for k in STATE_F64:
        if k in ('mean', 'm2'):
            continue
        assert np.array_equal(bits(host(d[k])), bits(getattr(st, k))), k
    for k in STATE_INT:
        assert np.array_equal(host(d[k]), getattr(st, k)), k
    assert np.all(np.isnan(host(d['z'])[st.Mcap:]))
    # Welford's sums: the host statement's, and the moments of the recorded states
    states = np.array(states)
    finite = np.all(np.isfinite(states), axis=(0, 2))
    size = np.max(np.abs(states), axis=0)
    for got, want, direct, power in ((host(d['mean']), st.mean, states.mean(axis=0), 1),
                                     (host(d['m2']), st.m2, states.var(axis=0) * NCALLS, 2)):
        assert np.all(np.abs(got - want)[finite] <= 1e-13 * np.abs(want)[finite])
        assert np.all(np.abs(got - direct)[finite] <= 1e-13 * NCALLS * size[finite]**power)
    assert np.array_equal(host(d['nstat']), np.full(nw, NCALLS))


def test_accept_refusals(eng):
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    st = sc.accept_case(3, 5, 4, 1)
    d = upload_state(eng, st)
    p = [_ptr(d['theta']), _ptr(d['logp']), _ptr(d['theta']), _ptr(d['logp']), _ptr(d['logp']),
         _ptr(d['rows']), _ptr(d['row_logp']), _ptr(d['row_gen']), _ptr(d['counts']),
         _ptr(d['nrows']), _ptr(d['overflow']), _ptr(d['mean']), _ptr(d['m2']), _ptr(d['nstat']),
         _ptr(d['z']), _ptr(d['nrows'])]
    with pytest.raises(_capi.PbError, match=r'generation 4294967296: the counter holds'):
        _capi.call('pb_demc_accept', *p, 2**32, 0, 4, 24, 0, 4, 3, 5, _stream())
    with pytest.raises(_capi.PbError, match='does not fit row_gen'):
        _capi.call('pb_demc_accept', *p, 2**31, 0, 4, 24, 0, 4, 3, 5, _stream())
    with pytest.raises(_capi.PbError, match='appending 5 rows to a history of 20: its capacity '
                                            'is 24'):
        _capi.call('pb_demc_accept', *p, 1, 0, 20, 24, 1, 4, 3, 5, _stream())
    with pytest.raises(_capi.PbError, match='null pointer'):
        _capi.call('pb_demc_accept', *p[:15], None, 1, 0, 4, 24, 0, 4, 3, 5, _stream())
    _capi.call('pb_demc_accept', *([None] * 16), 1, 0, 4, 24, 0, 4, 3, 0, _stream())


# -------------------------------------------------------------------------------------------------
# pb_gelman_rubin, pb_philox_uniform
# -------------------------------------------------------------------------------------------------
def run_rhat(eng, mean, m2, n):
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    nw, nfree = mean.shape
    out = nan_tensor((nfree + 1,))
    out[:nfree] = 7.0
    mean_d, m2_d = eng.dev(mean), eng.dev(m2)
    _capi.call('pb_gelman_rubin', _ptr(out), _ptr(mean_d), _ptr(m2_d), n, nfree, nw, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[nfree]))
    return host(out[:nfree])


def test_gelman_rubin(eng):
    from pyratbay_amd import sampler
    st = sc.gaussian_run_host(0, 200)
    chain = np.array(st.chain)[1:]                               # [200, 16, 3]
    got = run_rhat(eng, st.mean, st.m2, 200)
    np.testing.assert_allclose(got, sampler.gelman_rubin_host(st.mean, st.m2, 200), rtol=1e-12)
    W = chain.var(axis=0, ddof=1).mean(axis=0)
    B_over_n = chain.mean(axis=0).var(axis=0, ddof=1)
    np.testing.assert_allclose(got, np.sqrt((199 / 200 * W + B_over_n) / W), rtol=1e-12)
    assert np.all(got > 1.0) and np.all(got < 2.0)
    assert np.all(np.isnan(run_rhat(eng, st.mean[:1], st.m2[:1], 200)))
    assert np.all(np.isnan(run_rhat(eng, st.mean, st.m2, 1)))
    flat = st.m2.copy()
    flat[:, 1] = 0.0
    assert list(np.isnan(run_rhat(eng, st.mean, flat, 200))) == [False, True, False]
    # many parameters and chains: more than one block
    rng = np.random.default_rng(2)
    mean, m2 = rng.normal(0, 1, (65, 128)), rng.uniform(1, 2, (65, 128))
    np.testing.assert_allclose(run_rhat(eng, mean, m2, 9),
                               sampler.gelman_rubin_host(mean, m2, 9), rtol=1e-12)


@pytest.mark.parametrize('n,ncol', [(1, 1), (7, 5), (300, 128), (1000, 3)])
def test_philox_uniform_bits(eng, n, ncol):
    import torch
    from pyratbay_amd import _capi, sampler
    from pyratbay_amd._device import _ptr, _stream
    out = nan_tensor((n + 1, ncol))
    for seed in (0, SEED, 2**64 - 1):
        _capi.call('pb_philox_uniform', _ptr(out), seed, n, ncol, _stream())
        got = host(out)
        assert np.all(np.isnan(got[n]))
        assert np.array_equal(bits(got[:n]), bits(sampler.uniforms_host(seed, n, ncol)))
    with pytest.raises(_capi.PbError, match='null pointer'):
        _capi.call('pb_philox_uniform', None, 0, n, ncol, _stream())
    _capi.call('pb_philox_uniform', None, 0, 0, ncol, _stream())
    assert torch.isnan(out[n]).all()


# -------------------------------------------------------------------------------------------------
# the loop on the device against the loop on the host
# -------------------------------------------------------------------------------------------------
def gaussian_demc(eng, seed=0, capacity=201):
    theta0, z0 = sc.gaussian_start(seed)
    demc = eng.DEMC(sc.log_post_torch(), 3, sc.RUN_KW['pstep'], seed=seed,
                    fepsilon=sc.RUN_KW['fepsilon'])
    return demc.start(theta0, z0, capacity)


def no_read_back(fn):
    """Run fn with the read-backs of torch spied on; -> how many happened."""
    import torch
    reads = []
    names = ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__int__', '__float__')
    real = {n: getattr(torch.Tensor, n) for n in names}

    def spy(name):
        def wrapped(self, *a, **k):
            reads.append(name)
            return real[name](self, *a, **k)
        return wrapped
    for n in names:
        setattr(torch.Tensor, n, spy(n))
    try:
        fn()
    finally:
        for n in names:
            setattr(torch.Tensor, n, real[n])
    return reads


def test_device_loop_against_the_host_loop(eng):
    import torch
    want = sc.gaussian_run_host(0, 200)
    margin = np.array(want.margin)
    assert np.all(np.abs(margin[np.isfinite(margin)]) > 1e-9)
    demc = gaussian_demc(eng)
    accepted, states = [], [demc.theta.clone()]
    for _ in range(200):
        demc.run(1)
        accepted.append(demc.accepted.clone())
        states.append(demc.theta.clone())
    accepted = host(torch.stack(accepted))
    states = host(torch.stack(states))
    assert np.array_equal(accepted, np.array(want.accepted))
    assert np.all(np.abs(states - np.array(want.chain)) <= 1e-10 * sc.SIGMA)
    assert demc.M == want.M == 160 + 16 * 20 and demc.g == 200
    np.testing.assert_allclose(host(demc.rhat()),
                               eng.sampler.gelman_rubin_host(want.mean, want.m2, 200), rtol=1e-9)
    assert np.array_equal(host(demc.acceptance()), (want.nrows - 1) / 200.0)
    # one run of 200, launches only; and 120 + 80: the same bits
    whole = gaussian_demc(eng)
    assert no_read_back(lambda: whole.run(200)) == []
    parts = gaussian_demc(eng).run(120).run(80)
    for name in ('theta', 'logp', 'mean', 'm2', 'z', 'row_gen', 'counts', 'nrows', 'nstat'):
        assert torch.equal(getattr(parts, name), getattr(whole, name)), name
        assert torch.equal(getattr(demc, name), getattr(whole, name)), name
    used = torch.arange(201, device='cuda')[None, :] < whole.nrows[:, None]
    assert torch.equal(parts.rows[used], whole.rows[used])
    assert torch.equal(parts.row_logp[used], whole.row_logp[used])
    # unique: everything, and the last 150 generations of the host's chain
    theta, counts = whole.unique()
    assert counts.dtype == torch.int64 and int(counts.sum()) == 201 * 16
    assert theta.shape == (int(whole.nrows.sum()), 3)
    theta, counts = whole.unique(burn=50)
    expanded = np.repeat(host(theta), host(counts), axis=0)
    last = np.array(want.chain)[51:].transpose(1, 0, 2).reshape(-1, 3)
    assert expanded.shape == last.shape == (150 * 16, 3)
    assert np.all(np.abs(expanded - last) <= 1e-10 * sc.SIGMA)
    host_theta, host_counts = eng.sampler.unique_host(want, burn=50)
    assert np.array_equal(host(counts), host_counts)
    # a store without room says so
    tight = gaussian_demc(eng, capacity=8).run(200)
    assert bool((tight.overflow != 0).any()) and bool(torch.isnan(tight.acceptance()).any())
    with pytest.raises(ValueError, match='overflowed their store of 8 rows'):
        tight.unique()


def test_device_loop_refusals(eng):
    theta0, z0 = sc.gaussian_start(0)
    demc = eng.DEMC(sc.log_post_torch(), 3, sc.RUN_KW['pstep'])
    with pytest.raises(ValueError, match='start'):
        demc.run(1)
    bad = theta0.copy()
    bad[[1, 7]] = sc.MU - 11 * sc.SIGMA
    with pytest.raises(ValueError, match=r'chains \[1, 7\] have no finite log-posterior'):
        demc.start(bad, z0, 10)
    with pytest.raises(ValueError, match='a history of 2 rows'):
        demc.start(theta0, z0[:2], 10)
    with pytest.raises(ValueError, match='log_post must return a float64 device tensor'):
        eng.DEMC(lambda t: t[:, 0].float(), 3, sc.RUN_KW['pstep']).start(theta0, z0, 10)


def test_device_loop_samples_the_target(eng):
    """3000 generations at seed 0 on the device: the bounds committed for the host statement."""
    demc = gaussian_demc(eng, capacity=sc.NGEN + 1).run(sc.NGEN)
    theta, counts = demc.unique(burn=sc.BURN)
    assert int(counts.sum()) == (sc.NGEN - sc.BURN) * sc.NCHAINS
    mean, std, corr = sc.statistics(host(theta), host(counts).astype(float))
    acc = float(demc.acceptance().mean())
    rhat = host(demc.rhat())
    print(f'acceptance {acc:.3f}, worst |mean - mu| / sigma {mean:.4f}, worst relative error of '
          f'sigma {std:.4f}, worst correlation error {corr:.4f}, rhat {rhat}')
    assert sc.ACCEPTANCE[0] < acc < sc.ACCEPTANCE[1]
    assert mean <= sc.BOUND_MEAN and std <= sc.BOUND_STD and corr <= sc.BOUND_CORR
    assert np.all(rhat < 1.05)


# -------------------------------------------------------------------------------------------------
# Retrieval.draw_initial / sample / summary
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def retrieval(eng, golden):
    return sc.emission_retrieval(eng, golden)


def test_draw_initial(eng, retrieval):
    from pyratbay_amd import sampler
    ret = retrieval
    got = host(ret.draw_initial(80, seed=9))
    cube = sampler.uniforms_host(9, 80, ret.nfree)
    want = ret.prior_transform_host(cube)
    f = ret.ifree
    gauss = (ret.priorlow[f] != 0) | (ret.priorup[f] != 0)
    assert gauss.sum() == 2 and np.array_equal(bits(got[:, ~gauss]), bits(want[:, ~gauss]))
    # (test_gpu_retrieval's bound of the transform: 8 eps (|prior| + s (1 + |z|)), |z| < 6 here)
    s = np.maximum(ret.priorlow[f], ret.priorup[f])
    assert np.all(np.abs(got - want)[:, gauss] <= 8 * EPS * (np.abs(ret.prior[f]) + 7 * s)[gauss])
    assert np.all(ret.inside_host(got))
    # the default history of sample(): these draws, the chains starting from the last of them
    demc = ret.sample(sc.E2E_CHAINS, 2, seed=9)
    assert np.array_equal(bits(host(demc.z[:80])), bits(got))
    assert np.array_equal(bits(host(demc.rows[:, 0])), bits(got[-sc.E2E_CHAINS:]))
    assert demc.counts.sum(dim=1).tolist() == [3] * sc.E2E_CHAINS


def test_retrieval_sample_end_to_end(eng, retrieval):
    """8 chains x 30 generations against a host-driven loop: propose_host, the device's
    log_posterior, accept_host."""
    import torch
    from pyratbay_amd import sampler
    ret = retrieval
    nw, ngen, seed = sc.E2E_CHAINS, sc.E2E_NGEN, 5
    z0 = sc.emission_history(ret, 3)
    pstep = ret.pstep[ret.ifree]
    demc = ret.sample(nw, ngen, seed=seed, z0=z0, thin_z=5)
    assert demc.g == ngen and demc.M == 80 + nw * 6 and not bool(demc.overflow.any())

    def log_post(theta):
        return host(ret.log_posterior(eng.dev(theta)))
    theta0 = z0[-nw:].copy()
    st = sampler.new_state_host(theta0, log_post(theta0), z0, ngen + 1, thin_z=5)
    for g in range(1, ngen + 1):
        prop, log_jac, _ = sampler.propose_host(st.theta, st.z, st.M, pstep, g, seed)
        logp_prop = log_post(prop)
        margin = sampler.accept_margin_host(st.logp, logp_prop, log_jac, g, seed)
        assert np.all(np.abs(margin[np.isfinite(margin)]) > 1e-9)
        append = g % 5 == 0
        sampler.accept_host(st, prop, logp_prop, log_jac, g, seed, append)
        st.M += nw if append else 0
    assert 0 < st.nrows.sum() - nw < nw * ngen
    assert np.array_equal(host(demc.nrows), st.nrows)
    assert np.array_equal(host(demc.row_gen), st.row_gen)
    assert np.array_equal(host(demc.counts), st.counts)
    assert host(demc.counts).sum(axis=1).tolist() == [ngen + 1] * nw
    width = (ret.pmax - ret.pmin)[ret.ifree]
    assert np.all(np.isfinite(width))
    used = np.arange(ngen + 1)[None, :] < st.nrows[:, None]
    assert np.all(np.abs(host(demc.rows) - st.rows)[used] <= 1e-10 * width)
    assert np.all(np.abs(host(demc.theta) - st.theta) <= 1e-10 * width)
    assert np.all(np.abs(host(demc.z) - st.z[:demc.M]) <= 1e-10 * width)
    # the chain in the form posterior_summary takes
    theta, counts = demc.unique()
    assert int(counts.sum()) == (ngen + 1) * nw
    summary = ret.summary(demc)
    assert int(summary.n_rejected) == 0
    assert bool(torch.isfinite(summary.bands[0]).all()) and \
        bool(torch.isfinite(summary.spectrum[0]).all())
    trimmed = ret.summary(demc, burn=10)
    assert int(trimmed.n_rejected) == 0 and bool(torch.isfinite(trimmed.bands).all())
    # a starting state outside the bounds is refused before the loop
    bad = z0.copy()
    bad[-3, 0] = ret.pmin[ret.ifree][0] - 1.0
    calls = []
    real = ret.log_posterior
    ret.log_posterior = lambda t: (calls.append(t.shape[0]), real(t))[1]
    try:
        with pytest.raises(ValueError, match=r'chains \[5\] have no finite log-posterior'):
            ret.sample(nw, ngen, seed=seed, z0=bad)
    finally:
        del ret.log_posterior
    assert calls == [nw]
