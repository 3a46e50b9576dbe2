"""The NumPy statements of pyratbay_amd/sampler.py, which are the specification of the kernels in
csrc/pb_sampler.hip: Philox4x32-10 against the published known answers, the uniforms and the
index, the properties of a proposal, a run in two calls against one, the chain store against the
dense chain, and the statement doing its statistical job on a correlated Gaussian."""
import numpy as np
import pytest

import sampler_cases as sc
from pyratbay_amd import sampler


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_philox_known_answers():
    for counter, key, want in sc.KNOWN_ANSWERS:
        got = sampler.philox_host(counter, key)
        assert got.dtype == np.uint32 and [int(x) for x in got] == list(want)
    # vectorised: the three at once
    got = sampler.philox_host([c for c, _, _ in sc.KNOWN_ANSWERS],
                              [k for _, k, _ in sc.KNOWN_ANSWERS])
    assert np.array_equal(got, np.array([w for _, _, w in sc.KNOWN_ANSWERS], np.uint32))
    # the key is the seed, low word first; the counter is (block, chain, generation, tag)
    seed = (0x299f31d0 << 32) | 0xa4093822
    assert np.array_equal(sampler.block_host(seed, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
                          got[2])


def test_uniforms_and_index():
    assert sampler.u01_host(0, 0) == 2.0**-53
    assert sampler.u01_host(0xffffffff, 0xffffffff) == 1.0 - 2.0**-53
    # the six low bits of either word do not enter
    assert sampler.u01_host(0x3f, 0x3f) == 2.0**-53
    assert sampler.u01_host(0x40, 0) == (2.0**26 + 0.5) * 2.0**-52
    top = 1.0 - 2.0**-53
    assert sampler.index_host(top, 2**30) == 2**30 - 1
    assert sampler.index_host(2.0**-53, 2**30) == 0
    assert sampler.index_host(1.0, 2**30) == 2**30 - 1          # (the clamp; no u reaches 1)
    assert list(sampler.index_host(np.array([0.0, 0.34, 0.67, top]), 3)) == [0, 1, 2, 2]
    u = sampler.uniforms_host(5, 7, 5)
    assert u.shape == (7, 5) and np.all((u > 0) & (u < 1))
    ua, ub = sampler.block_uniforms_host(5, 1, 3, 0, sampler.TAG_INITIAL)
    assert u[3, 2] == ua and u[3, 3] == ub
    # a fair generator: mean and variance of 4e4 draws
    big = sampler.uniforms_host(1, 200, 200)
    assert abs(big.mean() - 0.5) < 4 * np.sqrt(1 / 12 / big.size)
    n = sampler.normals_host(1, np.arange(200), 9, 200)
    assert abs(n.mean()) < 4 / np.sqrt(n.size) and abs(n.var() - 1) < 4 * np.sqrt(2 / n.size)
    with pytest.raises(ValueError, match='2\\^32'):
        sampler.propose_host(np.zeros((1, 2)), np.ones((3, 2)), 3, np.ones(2), 2**32, 0)


@pytest.mark.parametrize('nfree', [1, 2, 7])
def test_propose_properties(nfree):
    nw, M = 400, 11
    theta, z, pstep, g = sc.propose_case(nfree, nw, M, 40 + nfree)
    prop, log_jac, kind, d = sampler.propose_host(theta, z, M, pstep, g, 3, fgamma=sc.FGAMMA,
                                                  fepsilon=0.0, p_snooker=sc.P_SNOOKER,
                                                  details=True)
    assert np.all(d.r1 != d.r2) and np.all((d.r1 >= 0) & (d.r1 < M))
    assert np.all((d.r2 >= 0) & (d.r2 < M)) and np.all((d.rz >= 0) & (d.rz < M))
    assert set(d.r1) == set(range(M)) and set(d.r2) == set(range(M))
    par, snk = kind == 0, kind == 1
    assert np.array_equal(snk, d.u_s < sc.P_SNOOKER) and par.sum() > 100 and snk.sum() > 100
    assert np.all(np.isfinite(prop)) and not np.any(np.isnan(log_jac))
    gamma = sc.FGAMMA * 2.38 / np.sqrt(2.0 * nfree)
    want = theta + gamma * (z[d.r1] - z[d.r2])
    assert np.array_equal(bits(prop[par]), bits(want[par])) and np.all(log_jac[par] == 0.0)
    # with fepsilon the normals enter
    eps_prop = sampler.propose_host(theta, z, M, pstep, g, 3, fgamma=sc.FGAMMA, fepsilon=0.05,
                                    p_snooker=sc.P_SNOOKER)[0]
    assert np.array_equal(bits(eps_prop[par]), bits((want + (0.05 * pstep) * d.normals)[par]))
    assert np.array_equal(bits(eps_prop[snk]), bits(prop[snk]))
    # a snooker proposal lies on the line through theta and Z[rz]
    a, b = (prop - theta)[snk], (theta - z[d.rz])[snk]
    cos = np.sum(a * b, axis=1) / np.sqrt(np.sum(a * a, axis=1) * np.sum(b * b, axis=1))
    assert np.all(np.abs(np.abs(cos) - 1.0) < 1e-12)
    if nfree == 1:
        assert np.all(log_jac == 0.0)
    else:
        ratio = np.sum((prop - z[d.rz])**2, axis=1) / np.sum((theta - z[d.rz])**2, axis=1)
        assert np.allclose(log_jac[snk], 0.5 * (nfree - 1) * np.log(ratio[snk]), rtol=1e-12,
                           atol=1e-12)
        assert np.any(log_jac[snk] != 0.0)


def test_propose_degenerate_history():
    """Every row of the history equals the walker: prop = theta, log_jac = 0, either kind."""
    theta = np.tile(np.array([[0.3, -1.5, 2.0e3]]), (64, 1))
    z = np.tile(theta[:1], (5, 1))
    prop, log_jac, kind = sampler.propose_host(theta, z, 5, np.ones(3), 7, 1, p_snooker=0.5)
    assert set(kind) == {0, 1}
    assert np.array_equal(bits(prop), bits(theta)) and np.all(log_jac == 0.0)
    with pytest.raises(ValueError, match='at least 3'):
        sampler.propose_host(theta, z, 2, np.ones(3), 7, 1)


def small_run(ngen, state=None, capacity=None):
    theta0, z0 = sc.gaussian_start(3)
    return sampler.run_host(sc.log_post_host, theta0, z0, ngen, seed=3, thin_z=4,
                            capacity=capacity, state=state, **sc.RUN_KW)


def test_run_in_two_calls_equals_one():
    whole = small_run(90)
    cap = whole.cap
    parts = small_run(40, small_run(50, capacity=cap))
    assert parts.g == whole.g == 90 and parts.M == whole.M == 160 + 16 * 22
    for name in ('theta', 'logp', 'rows', 'row_logp', 'mean', 'm2', 'z'):
        assert np.array_equal(bits(getattr(parts, name)), bits(getattr(whole, name))), name
    for name in ('row_gen', 'counts', 'nrows', 'overflow', 'nstat'):
        assert np.array_equal(getattr(parts, name), getattr(whole, name)), name
    assert np.array_equal(bits(np.array(parts.chain)), bits(np.array(whole.chain)))


def test_chain_store_against_the_dense_chain():
    st = small_run(90)
    chain = np.array(st.chain)                                   # [91, nw, 3]
    accepted = np.array(st.accepted)
    assert 0.1 < accepted.mean() < 0.6 and not np.any(st.overflow)
    expanded = sampler.expand_host(st.rows, st.counts, st.nrows)
    for w in range(chain.shape[1]):
        assert np.array_equal(bits(expanded[w]), bits(chain[:, w]))
        # a row begins where the chain accepted
        assert list(st.row_gen[w, 1:st.nrows[w]]) == list(1 + np.where(accepted[:, w])[0])
    assert np.array_equal(st.nrows - 1, accepted.sum(axis=0))
    assert np.array_equal(st.logp, sc.log_post_host(st.theta))
    # the history: z0, then the states after every fourth generation
    assert np.array_equal(bits(st.z[160:160 + 16 * 22]),
                          bits(chain[4:89:4].reshape(-1, 3)))
    # Welford's sums are the moments of the samples 1 .. 90
    assert np.allclose(st.mean, chain[1:].mean(axis=0), rtol=1e-13, atol=1e-15)
    assert np.allclose(st.m2, chain[1:].var(axis=0) * 90, rtol=1e-12)
    rhat = sampler.gelman_rubin_host(st.mean, st.m2, 90)
    W = chain[1:].var(axis=0, ddof=1).mean(axis=0)
    B_over_n = chain[1:].mean(axis=0).var(axis=0, ddof=1)
    assert np.allclose(rhat, np.sqrt((89 / 90 * W + B_over_n) / W), rtol=1e-12)
    assert np.all(np.isnan(sampler.gelman_rubin_host(st.mean[:1], st.m2[:1], 90)))
    assert np.all(np.isnan(sampler.gelman_rubin_host(st.mean, st.m2, 1)))
    assert np.all(np.isnan(sampler.gelman_rubin_host(st.mean, 0 * st.m2, 90)))
    # unique: everything; and the last 40 generations
    theta, counts = sampler.unique_host(st)
    assert counts.sum() == 91 * 16 and len(theta) == st.nrows.sum()
    theta, counts = sampler.unique_host(st, burn=50)
    assert np.array_equal(bits(np.repeat(theta, counts, axis=0)),
                          bits(chain[51:].transpose(1, 0, 2).reshape(-1, 3)))
    # a store without room: the flag, no more recording, the same states
    # (its history has room for one append only: 160 + 16 (5 // 4) rows)
    tight = small_run(90, capacity=5)
    assert tight.M == tight.Mcap == 176 and tight.g == 90
    dense, took = np.array(tight.chain), np.array(tight.accepted)
    over = tight.overflow != 0
    assert np.any(over) and np.all(tight.nrows[over] == 5)
    assert np.array_equal(over, took.sum(axis=0) > 4)
    for w in range(16):
        gens = 1 + np.where(took[:, w])[0]
        k = tight.nrows[w]
        assert np.array_equal(bits(tight.rows[w, :k]), bits(dense[np.r_[0, gens[:k - 1]], w]))
        # the counts stop at the accept that found no room
        assert tight.counts[w, :k].sum() == (gens[4] if over[w] else 91)
    with pytest.raises(ValueError, match='overflowed'):
        sampler.unique_host(tight)


def test_starting_states_are_checked():
    theta0, z0 = sc.gaussian_start(3)
    theta0[[2, 5]] = sc.MU + 11 * sc.SIGMA
    with pytest.raises(ValueError, match=r'chains \[2, 5\]'):
        sampler.run_host(sc.log_post_host, theta0, z0, 1)


def test_the_statement_samples_the_target():
    """16 chains x 3000 generations at seed 0, burn 500, on the correlated Gaussian: mean,
    standard deviation and correlation within the committed bounds (twice the worst of seeds
    0 - 19, profiles/sampler.md)."""
    st = sc.gaussian_run_host(0, sc.NGEN)
    acc = float(np.mean(st.accepted))
    theta, counts = sampler.unique_host(st, sc.BURN)
    assert counts.sum() == (sc.NGEN - sc.BURN) * sc.NCHAINS
    mean, std, corr = sc.statistics(theta, counts)
    rhat = sampler.gelman_rubin_host(st.mean, st.m2, sc.NGEN)
    print(f'acceptance {acc:.3f}, worst |mean - mu| / sigma {mean:.4f}, worst relative error of '
          f'sigma {std:.4f}, worst correlation error {corr:.4f}, rhat {rhat}')
    assert sc.ACCEPTANCE[0] < acc < sc.ACCEPTANCE[1]
    assert mean <= sc.BOUND_MEAN and std <= sc.BOUND_STD and corr <= sc.BOUND_CORR
    assert np.all(rhat < 1.05)
