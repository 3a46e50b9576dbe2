"""The NumPy statements of the nested sampler (pyratbay_amd/nested.py), which are the
specification of csrc/pb_nested.hip: select on hand-made log-likelihoods, the constraints of the
walk, continuation, the evidence of a Gaussian whose value is known in closed form (20 seeds,
profiles/nested.md), the finish sums and the resampling."""
import os

import numpy as np
import pytest

import nested_cases as nc
from pyratbay_amd import nested, sampler


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# -------------------------------------------------------------------------------------------------
# select
# -------------------------------------------------------------------------------------------------
def test_select_order_on_special_values():
    logl = nc.special_logl()
    #        0     1      2     3    4     5     6    7     8      9    10    11
    #      -3.0  -1e98  -7.5  NaN  -3.0  -inf   2.0  -7.5  -1e98  -3.0  0.5  -inf
    order = [3, 5, 11, 1, 8, 2, 7, 0, 4, 9, 10, 6]
    assert list(nested.rank_host(logl)) == order
    for K in (1, 2, 5, 10):
        sel = nested.select_host(logl, 0.0, -np.inf, K)
        assert list(sel.dead_idx) == order[:K] and list(sel.surv_idx) == order[K:]
        assert np.array_equal(bits(sel.dead_logl), bits(logl[order[:K]]))
        assert sel.ln_x == -np.cumsum(1.0 / (12 - np.arange(K)))[-1]
        np.testing.assert_allclose(sel.ln_x, -np.sum(1.0 / (12 - np.arange(K))), rtol=1e-15)
        # a NaN and a -inf weigh nothing; -1e98 weighs exp(-1e98)
        assert np.all(sel.dead_logw[:min(K, 3)] == -np.inf)
        assert bits(sel.lstar) == bits(logl[order[K - 1]])
    assert sel.ln_z == pytest.approx(np.logaddexp.reduce(sel.dead_logw), rel=1e-13)
    # two NaNs: by index, both below -inf
    assert list(nested.rank_host([np.nan, -np.inf, np.nan, 1.0])) == [0, 2, 1, 3]
    for K, nlive in ((0, 12), (11, 12), (1, 2)):
        with pytest.raises(ValueError, match='1 <= batch <= nlive - 2'):
            nested.select_host(np.zeros(nlive), 0.0, -np.inf, K)
    with pytest.raises(ValueError, match='4097 live points: at most 4096'):
        nested.select_host(np.zeros(4097), 0.0, -np.inf, 1)


@pytest.mark.parametrize('nlive', [5, 64, 300])
def test_select_weights(nlive):
    rng = np.random.default_rng(nlive)
    logl = rng.normal(-20.0, 5.0, nlive)
    ln_x0, ln_z0 = -0.75, -31.0
    for K in nc.batches(nlive):
        sel = nested.select_host(logl, ln_x0, ln_z0, K)
        assert np.all(np.diff(sel.dead_logl) >= 0)
        assert sel.dead_logl[-1] <= np.min(logl[sel.surv_idx])
        n = nlive - np.arange(K)
        x_before = np.exp(ln_x0 - np.concatenate(([0.0], np.cumsum(1.0 / n)[:-1])))
        x_after = np.exp(ln_x0 - np.cumsum(1.0 / n))
        direct = np.log(x_before - x_after) + sel.dead_logl
        assert np.all(np.abs(sel.dead_logw - direct) <= 1e-13 * np.abs(direct))
        want_z = np.logaddexp.reduce(np.concatenate(([ln_z0], sel.dead_logw)))
        assert abs(sel.ln_z - want_z) <= 1e-13 * abs(want_z)
        assert abs(sel.ln_x - (ln_x0 - np.sum(1.0 / n))) <= 1e-14
        top = np.max(logl[sel.surv_idx])
        assert sel.remain == pytest.approx(np.logaddexp(sel.ln_z, top + sel.ln_x) - sel.ln_z,
                                           rel=1e-13)
        assert sel.remain > 0


# -------------------------------------------------------------------------------------------------
# the walk
# -------------------------------------------------------------------------------------------------
def test_start_and_propose_draw_survivors_only():
    rng = np.random.default_rng(3)
    nlive, K, nfree = 40, 9, 4
    live_u = rng.uniform(0.3, 0.7, (nlive, nfree))
    live_logl = rng.normal(0, 1, nlive)
    surv_idx = rng.permutation(nlive)[:nlive - K]
    dead = sorted(set(range(nlive)) - set(surv_idx))
    # a row nobody may read
    live_u[dead] = np.nan
    seen_a, seen_b, unit = set(), set(), 0
    for q in range(200):
        cur, cur_logl, pick = nested.start_host(live_u, live_logl, surv_idx, K, q + 1, 5)
        assert set(pick) <= set(surv_idx) and np.array_equal(bits(cur), bits(live_u[pick]))
        assert np.array_equal(bits(cur_logl), bits(live_logl[pick]))
        point, inside, d = nested.propose_host(cur, live_u, surv_idx, q, 5, nc.FGAMMA,
                                               nc.P_UNIT, details=True)
        assert np.all(d.a != d.b) and np.all((d.a >= 0) & (d.a < nlive - K))
        assert np.all((d.b >= 0) & (d.b < nlive - K))
        assert np.all(np.isfinite(d.prop))
        seen_a |= set(d.a)
        seen_b |= set(d.b)
        unit += int(np.sum(d.gamma == 1.0))
        assert set(d.gamma) <= {1.0, sampler.gamma_host(nc.FGAMMA, nfree)}
        want = cur + d.gamma[:, None] * (live_u[surv_idx[d.a]] - live_u[surv_idx[d.b]])
        assert np.array_equal(bits(d.prop), bits(want))
        want_inside = np.all((want > 0) & (want < 1), axis=1)
        assert np.array_equal(inside, want_inside.astype(np.int32))
        assert np.array_equal(bits(point), bits(np.where(want_inside[:, None], want, cur)))
    assert seen_a == seen_b == set(range(nlive - K))
    assert 0.2 < unit / (200.0 * K) < 0.4
    for what, call in (('q', lambda: nested.propose_host(cur, live_u, surv_idx, 2**32, 5)),
                       ('it', lambda: nested.start_host(live_u, live_logl, surv_idx, K, 2**32, 5))):
        with pytest.raises(ValueError, match=f'{what} 4294967296: the counter holds'):
            call()


def test_the_propose_cases_fall_on_both_sides_of_the_cube():
    """The calls the GPU test makes: over each (nfree, K) both values of inside occur, and an
    outside slot carries cur (propose_expectations asserts the first itself)."""
    for nfree in nc.NFREES:
        for K in nc.KS:
            for c in nc.propose_expectations(nfree, K):
                out = c['inside'] == 0
                assert np.array_equal(bits(c['point'][out]), bits(c['cur'][out]))
                assert np.array_equal(bits(c['point'][~out]), bits(c['prop'][~out]))


def test_accept_rules():
    st = nc.accept_case(3, 6, 1)
    lstar = -10.0
    cur0, logl0 = st.cur.copy(), st.cur_logl.copy()
    live0 = st.live_u.copy()
    point = np.full((6, 3), 0.5)
    #                  outside  NaN     equal   above   below   +inf
    logl = np.array([1e300, np.nan, lstar, -9.999, -10.001, np.inf])
    inside = np.array([0, 1, 1, 1, 1, 1], np.int32)
    acc = nested.accept_host(st, point, logl, inside, lstar)
    assert list(acc) == [0, 0, 0, 1, 0, 1]
    assert np.array_equal(bits(st.cur[acc == 0]), bits(cur0[acc == 0]))
    assert np.array_equal(bits(st.cur_logl[acc == 0]), bits(logl0[acc == 0]))
    assert np.all(st.cur[acc == 1] == 0.5) and list(st.cur_logl[acc == 1]) == [-9.999, np.inf]
    assert list(st.naccept) == list(st.acc_it) == [0, 0, 0, 1, 0, 1]
    assert np.array_equal(bits(st.live_u), bits(live0)) and not st.stuck.any()
    # a NaN threshold accepts nothing
    assert not nested.accept_host(st, point, np.zeros(6), np.ones(6, np.int32), np.nan).any()
    # the last step: the slots go home, and those that never moved are counted
    acc = nested.accept_host(st, point, logl, np.zeros(6, np.int32), lstar, st.dead_idx)
    assert not acc.any() and list(st.stuck) == [1, 1, 1, 0, 1, 0]
    assert np.array_equal(bits(st.live_u[st.dead_idx]), bits(st.cur))
    assert np.array_equal(bits(st.live_logl[st.dead_idx]), bits(st.cur_logl))
    others = np.setdiff1d(np.arange(len(live0)), st.dead_idx)
    assert np.array_equal(bits(st.live_u[others]), bits(live0[others]))


def run_small(niter, state=None, **kw):
    return nested.run_host(nc.log_like_host, nc.prior_transform_host, 64, 16, 8, niter, seed=7,
                           nfree=3, state=state, **kw)


def test_continuation_has_the_bits_of_one_run():
    whole = run_small(15)
    parts = run_small(6, state=run_small(9))
    assert whole.it == parts.it == 15 and len(whole.dead_logl) == 15 * 16
    for name in ('live_u', 'live_logl', 'dead_u', 'dead_logl', 'dead_logw', 'cur', 'cur_logl'):
        assert np.array_equal(bits(getattr(whole, name)), bits(getattr(parts, name))), name
    for name in ('ln_x', 'ln_z', 'lstar', 'remain'):
        assert bits(getattr(whole, name)) == bits(getattr(parts, name)), name
    for name in ('naccept', 'stuck'):
        assert np.array_equal(getattr(whole, name), getattr(parts, name))
    assert np.array_equal(np.array(whole.accepted), np.array(parts.accepted))
    # every live point lies above the last threshold, the dead ones rise
    assert np.all(whole.live_logl > whole.lstar) or whole.stuck.sum() > 0
    assert np.all(np.diff(whole.dead_logl.reshape(15, 16), axis=1) >= 0)
    assert np.all(np.diff(whole.dead_logl.reshape(15, 16)[:, -1]) > 0)
    # nothing outside the cube is ever stored
    assert np.all((whole.dead_u > 0) & (whole.dead_u < 1))
    assert np.all((whole.live_u > 0) & (whole.live_u < 1))
    assert np.array_equal(bits(whole.dead_u[:16]),
                          bits(sampler.uniforms_host(7, 64, 3)[whole.dead_idx[0]]))
    # dlogz: stops at the first iteration that leaves less
    early = run_small(15, dlogz=whole.remain * 1.0000001)
    assert early.it <= 15 and early.remain < whole.remain * 1.0000001
    assert run_small(15, dlogz=1e-300).it == 15


# -------------------------------------------------------------------------------------------------
# the evidence of the Gaussian target
# -------------------------------------------------------------------------------------------------
def test_evidence_of_the_gaussian_target():
    """run_host at nlive 512, batch 128, nsteps 30, dlogz 0.01 over seeds 0 - 19 (the table is
    in profiles/nested.md): the worst figures are those the committed bounds were made from, the
    ln Z bound does not exceed 0.5, and the mean over the seeds agrees with the closed form."""
    assert nc.LN_Z == pytest.approx(-6.7412, abs=5e-5)
    assert nc.BOUND_LNZ <= 0.5
    lnz, err, stats, its = [], [], [], []
    for seed in nc.SEEDS:
        st = nc.gaussian_run_host(seed)
        assert st.remain < nc.DLOGZ and st.it < nc.MAX_ITER
        z, e, s, _ = nc.result_host(st, seed)
        lnz.append(z), err.append(e), stats.append(s), its.append(st.it)
    lnz, stats = np.array(lnz), np.array(stats)
    worst = np.max(np.abs(lnz - nc.LN_Z))
    std = np.std(lnz, ddof=1)
    print(f'worst |ln Z - analytic| {worst:.5f}; mean {np.mean(lnz):.4f} against {nc.LN_Z:.4f}, '
          f'std {std:.4f}, reported error {np.mean(err):.4f}; iterations {min(its)} - {max(its)}; '
          f'worst mean, sigma, correlation errors {np.max(stats, axis=0)}')
    assert worst <= nc.BOUND_LNZ
    assert abs(np.mean(lnz) - nc.LN_Z) <= 3.0 * std / np.sqrt(len(nc.SEEDS))
    assert np.all(np.max(stats, axis=0) <= (nc.BOUND_MEAN, nc.BOUND_STD, nc.BOUND_CORR))
    # the committed worst values are these runs' (the bounds are twice them)
    np.testing.assert_allclose((worst,) + tuple(np.max(stats, axis=0)),
                               (nc.WORST_LNZ, nc.WORST_MEAN, nc.WORST_STD, nc.WORST_CORR),
                               atol=1e-5)


# -------------------------------------------------------------------------------------------------
# finish and resample
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ndead,nlive', [(0, 3), (5, 4), (1000, 64), (5120, 512)])
def test_finish_against_direct_sums(ndead, nlive):
    dead_logl, dead_logw, live_logl, ln_x = nc.finish_case(ndead, nlive, ndead + nlive)
    fin = nested.finish_host(dead_logl, dead_logw, live_logl, ln_x)
    n = ndead + nlive
    assert fin.logw.shape == fin.logl.shape == fin.cdf.shape == (n,)
    with np.errstate(invalid='ignore'):
        live_logw = np.where(np.isnan(live_logl), -np.inf, live_logl + ln_x - np.log(nlive))
    logw = np.concatenate((dead_logw, live_logw))
    assert np.array_equal(bits(fin.logw), bits(logw))
    ln_z = np.logaddexp.reduce(logw)
    p = np.exp(logw - ln_z)
    info = np.sum(np.where(p > 0, p * np.where(p > 0, fin.logl, 0.0), 0.0)) - ln_z
    assert fin.ln_z == pytest.approx(ln_z, rel=1e-13)
    assert fin.info == pytest.approx(info, rel=1e-11)
    assert fin.ln_z_err == pytest.approx(np.sqrt(info / nlive), rel=1e-11)
    assert np.all(np.diff(fin.cdf) >= 0) and fin.cdf[-1] == pytest.approx(1.0, abs=1e-14)
    assert np.all(np.abs(fin.cdf - np.cumsum(p)) <= 1e-13)


def test_resample_counts():
    dead_logl, dead_logw, live_logl, ln_x = nc.finish_case(1000, 64, 5)
    fin = nested.finish_host(dead_logl, dead_logw, live_logl, ln_x)
    for nsamples in (0, 1, 7, 1064, 5000):
        counts = nested.resample_host(fin.cdf, nsamples, 9)
        u = nested.resample_uniforms_host(9, nsamples)
        assert counts.dtype == np.int64 and counts.sum() == nsamples
        want = np.bincount(np.searchsorted(fin.cdf, u, 'right'), minlength=len(fin.cdf))
        assert np.array_equal(counts, want)
        # rows without weight get nothing
        assert not counts[fin.logw == -np.inf].any()
    # the uniforms: both halves of a block, sample by sample
    ua, ub = sampler.block_uniforms_host(9, 0, np.arange(4), 0, nested.TAG_NESTED_RESAMPLE)
    assert np.array_equal(bits(u[:8]), bits(np.stack((ua, ub), axis=1).reshape(-1)))
    # a uniform at or above the last cdf value falls on the last row
    assert list(nested.resample_host([0.25, 0.5], 1000, 1)[:1]) != [1000]
    assert nested.resample_host([0.25, 0.5], 1000, 1).sum() == 1000
    with pytest.raises(ValueError, match='at most 2\\^32'):
        nested.resample_uniforms_host(0, 2**32 + 1)


@pytest.mark.parametrize('ndead,nlive', nc.FINISH_SHAPES)
def test_few_draws_come_near_a_cdf_value(ndead, nlive):
    """The device's cdf may differ from the host's in its last bits, so the GPU test compares
    counts only over the draws farther than 1e-12 from a cdf value; at its shapes and sample
    counts those are all but 1 % at the most, on the host alone."""
    dead_logl, dead_logw, live_logl, ln_x = nc.finish_case(ndead, nlive, ndead + nlive)
    fin = nested.finish_host(dead_logl, dead_logw, live_logl, ln_x)
    n = ndead + nlive
    seed = 0x1234567887654321
    for nsamples in nc.resample_counts(n):
        u = nested.resample_uniforms_host(seed + nsamples, nsamples)
        index, near = nc.near_cdf(fin.cdf, u)
        assert near.mean() <= 0.01
        assert np.array_equal(np.bincount(index, minlength=n),
                              nested.resample_host(fin.cdf, nsamples, seed + nsamples))


def test_defaults_and_refusals():
    assert nested.default_batch(1000) == 250 and nested.default_batch(4) == 1
    assert nested.default_nsteps(3) == 20 and nested.default_nsteps(11) == 55
    assert (nested.TAG_NESTED_START, nested.TAG_NESTED_STEP, nested.TAG_NESTED_RESAMPLE) == \
        (3, 4, 5)
    assert len({sampler.TAG_PROPOSE, sampler.TAG_ACCEPT, sampler.TAG_INITIAL, 3, 4, 5}) == 6
    with pytest.raises(ValueError, match='1 <= batch <= nlive - 2'):
        nested.NestedSampler(None, None, 3, 10, batch=9)
    with pytest.raises(ValueError, match='129 free parameters'):
        nested.NestedSampler(None, None, 129, 10)
    with pytest.raises(ValueError, match='at most 4096'):
        nested.NestedSampler(None, None, 3, 5000)
    ns = nested.NestedSampler(None, None, 11, 1000)
    assert (ns.K, ns.nsteps) == (250, 55)
    with pytest.raises(ValueError, match='start'):
        ns.run(1)


def test_the_library_exports_the_entries():
    from pyratbay_amd import _capi, engine
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(os.path.dirname(here), 'include', 'pbhip.h')).read()
    for name in ('pb_nested_select', 'pb_nested_propose', 'pb_nested_accept', 'pb_nested_finish',
                 'pb_nested_resample'):
        assert name in text and name in _capi.exported_names() and hasattr(_capi.lib(), name)
    assert engine.NestedSampler is nested.NestedSampler and engine.nested is nested
    assert callable(engine.Retrieval.nested)
