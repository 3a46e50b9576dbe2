"""Cases the nested sampler's CPU and GPU tests share (pyratbay_amd/nested.py,
csrc/pb_nested.hip): the Gaussian target of sampler_cases on the cube mapped to MU +- 10 SIGMA,
whose evidence is known in closed form, with its committed bounds; hand-made log-likelihoods for
select; inputs for the propose, accept and finish kernels."""
import functools

import numpy as np

import sampler_cases as sc

# -------------------------------------------------------------------------------------------------
# the Gaussian target: L = exp(_quadratic), a uniform prior over the box MU +- 10 SIGMA
# -------------------------------------------------------------------------------------------------
LN_Z = float(np.log((2.0 * np.pi)**1.5 * np.sqrt(1.0 - sc.RHO**2) / 20.0**3))     # -6.7412...
NLIVE, BATCH, NSTEPS, DLOGZ, MAX_ITER = 512, 128, 30, 0.01, 400
SEEDS = tuple(range(20))

# The worst values of run_host over seeds 0 - 19 at those settings (profiles/nested.md has the
# table), and the committed bounds: twice each, because 20 seeds sample the tail thinly.  Two
# conditions are not measurements: BOUND_LNZ may not exceed 0.5, and the mean of ln Z over the 20
# seeds lies within 3 std / sqrt(20) of LN_Z.  At nsteps = 20 the worst |ln Z - LN_Z| was 0.25822:
# twice that exceeds 0.5, so the walk was lengthened to 30 steps; the bounds were not widened.
WORST_LNZ, WORST_MEAN, WORST_STD, WORST_CORR = 0.22581, 0.05800, 0.04989, 0.07523
BOUND_LNZ, BOUND_MEAN, BOUND_STD, BOUND_CORR = (2 * WORST_LNZ, 2 * WORST_MEAN, 2 * WORST_STD,
                                                2 * WORST_CORR)


def prior_transform_host(cube):
    return sc.MU + (20.0 * np.asarray(cube) - 10.0) * sc.SIGMA


def log_like_host(theta):
    t = (np.asarray(theta) - sc.MU) / sc.SIGMA
    return sc._quadratic(t[:, 0], t[:, 1], t[:, 2])


def target_torch():
    """(log_like, prior_transform): the same operations as torch callables on device tensors."""
    import torch
    mu = torch.as_tensor(sc.MU, device='cuda')
    sigma = torch.as_tensor(sc.SIGMA, device='cuda')

    def prior_transform(cube):
        return mu + (20.0 * cube - 10.0) * sigma

    def log_like(theta):
        t = (theta - mu) / sigma
        return sc._quadratic(t[:, 0], t[:, 1], t[:, 2])
    return log_like, prior_transform


@functools.lru_cache(maxsize=None)
def gaussian_run_host(seed, nlive=NLIVE, batch=BATCH, nsteps=NSTEPS, niter=MAX_ITER, dlogz=DLOGZ):
    """run_host on the target (computed once per session; do not modify the result)."""
    from pyratbay_amd import nested
    return nested.run_host(log_like_host, prior_transform_host, nlive, batch, nsteps, niter,
                           seed=seed, nfree=3, dlogz=dlogz)


def result_host(st, seed):
    """(ln Z, ln Z_err, statistics of the resampled posterior, the finish namespace) of a state."""
    from pyratbay_amd import nested
    fin = nested.finish_host(st.dead_logl, st.dead_logw, st.live_logl, st.ln_x)
    counts = nested.resample_host(fin.cdf, len(fin.cdf), seed)
    theta = prior_transform_host(np.concatenate((st.dead_u, st.live_u)))
    keep = counts > 0
    return fin.ln_z, fin.ln_z_err, sc.statistics(theta[keep], counts[keep].astype(float)), fin


# -------------------------------------------------------------------------------------------------
# inputs of the kernels
# -------------------------------------------------------------------------------------------------
NLIVES = (3, 5, 64, 65, 300, 4096)
NFREES, KS = sc.NFREES, sc.NWS
FGAMMA, P_UNIT = 0.9, 0.3


def batches(nlive):
    return sorted({1, min(2, nlive - 2), nlive - 2})


def special_logl():
    """Hand-made: repeated values, -inf, the reject value -1e98 and a NaN."""
    return np.array([-3.0, -1e98, -7.5, np.nan, -3.0, -np.inf, 2.0, -7.5, -1e98, -3.0, 0.5,
                     -np.inf])


def select_logl(nlive, seed):
    """live_logl[nlive]: draws rounded to one decimal, so that values repeat, with a NaN, a -inf
    and a -1e98 among them where there is room (nlive >= 5)."""
    rng = np.random.default_rng(seed)
    logl = np.round(rng.normal(-20.0, 5.0, nlive), 1)
    if nlive >= 5:
        where = rng.choice(nlive, 4, replace=False)
        logl[where[0]] = np.nan
        logl[where[1]] = -np.inf
        logl[where[2]] = -1e98
        logl[where[3]] = logl[(where[3] + 1) % nlive]
    return logl


def propose_case(nfree, K, seed):
    """A live cube of 3 K + 7 points, K slots somewhere inside it, the survivors (a shuffled
    subset that leaves K points out) and a global step to start from.  The points sit in
    [0.25, 0.75] and the slots in [0.02, 0.98], so that proposals fall on both sides of the cube's
    faces for few parameters and the unit-gamma jumps leave it for many."""
    rng = np.random.default_rng(seed)
    nlive = 3 * K + 7
    live_u = rng.uniform(0.25, 0.75, (nlive, nfree))
    cur = rng.uniform(0.02, 0.98, (K, nfree))
    if nfree > 8:
        # many parameters: most slots near the centre (a jump of gamma 2.38 / sqrt(2 nfree) stays
        # inside), the others near a face
        cur[::2] = rng.uniform(0.45, 0.55, cur[::2].shape)
    surv_idx = rng.permutation(nlive)[:nlive - K].astype(np.int32)
    q = int(rng.integers(1, 2**31))
    return live_u, cur, surv_idx, nlive, q


def accept_case(nfree, K, seed):
    """A state (nested.new_state_host) of nlive = 2 K + 3 live points with K slots under way."""
    from pyratbay_amd import nested
    rng = np.random.default_rng(seed)
    nlive = 2 * K + 3
    st = nested.new_state_host(rng.uniform(0, 1, (nlive, nfree)), rng.uniform(-50, -1, nlive), K)
    st.cur = rng.uniform(0, 1, (K, nfree))
    st.cur_logl = rng.uniform(-20, -1, K)
    st.dead_idx = rng.permutation(nlive)[:K].astype(np.int32)
    return st


def accept_inputs(st, step, rng, lstar):
    """point, logl_prop, inside for one call: about half the slots above lstar, one in five
    outside the cube, special values every fourth step, and every finite margin
    |logl_prop - lstar| exceeds 1e-9 (asserted)."""
    K, nfree = st.cur.shape
    point = rng.uniform(0, 1, (K, nfree))
    logl_prop = lstar + rng.normal(0.0, 2.0, K)
    inside = (rng.uniform(0, 1, K) < 0.8).astype(np.int32)
    if step % 4 == 0:
        for j, k in enumerate(range(min(K, 3))):
            logl_prop[k] = (np.nan, -np.inf, np.inf)[(j + step // 4) % 3]
            inside[k] = 1
    margin = logl_prop - lstar
    finite = np.isfinite(margin)
    assert np.all(np.abs(margin[finite]) > 1e-9)
    return point, logl_prop, inside


def finish_case(ndead, nlive, seed):
    """dead_logl, dead_logw, live_logl, ln_x of a run that never happened but looks like one:
    logl rising, ln X falling by 1 / nlive per death, a NaN and a -inf at the start."""
    rng = np.random.default_rng(seed)
    dead_logl = np.sort(rng.normal(-30.0, 10.0, ndead))
    ln_x_j = -np.arange(ndead) / float(nlive)
    dead_logw = dead_logl + ln_x_j + np.log(-np.expm1(-1.0 / nlive))
    if ndead >= 2:
        dead_logl[0], dead_logw[0] = np.nan, -np.inf
        dead_logl[1], dead_logw[1] = -np.inf, -np.inf
    live_logl = (dead_logl[-1] if ndead else -30.0) + rng.exponential(3.0, nlive)
    if nlive >= 3:
        live_logl[2] = np.nan
    return dead_logl, dead_logw, live_logl, -ndead / float(nlive)


FINISH_SHAPES = [(0, 3), (5, 4), (1000, 64), (5120, 512), (70000, 4096)]


def resample_counts(n):
    """The numbers of samples the finish test draws over n rows."""
    return (n, 1, 4 * n + 3)


def near_cdf(cdf, u):
    """(index[len(u)], near[len(u)]): the row each uniform falls on (the first i with cdf[i] > u,
    clipped), and whether it comes within 1e-12 of the cdf value on either side of it: such a
    draw may fall on the neighbouring row under a cdf that differs in its last bits."""
    n = len(cdf)
    index = np.minimum(np.searchsorted(cdf, u, 'right'), n - 1)
    near = np.minimum(np.abs(u - cdf[index]), np.abs(u - cdf[np.maximum(index - 1, 0)])) <= 1e-12
    return index, near


PROPOSE_STEPS = {1: 12, 5: 4, 65: 2}


def propose_expectations(nfree, K, seed=0x1234567887654321):
    """The calls of the propose test and what propose_host says of them: a list of dicts with the
    inputs (live_u, live_logl, surv_idx, cur or None with the start flag, it, q) and the host's
    cur, cur_logl, point, inside, a, b, gamma.  Over the list both values of inside occur
    (asserted here, on the host)."""
    from pyratbay_amd import nested
    live_u, cur0, surv_idx, nlive, q0 = propose_case(nfree, K, 7 * nfree + 100 * K)
    live_logl = np.random.default_rng(K).normal(-10.0, 3.0, nlive)
    calls, seen = [], set()
    for i in range(PROPOSE_STEPS[K]):
        start = i % 2 == 0
        it, q = q0 // 3 + i, q0 + i
        if start:
            cur, cur_logl, _ = nested.start_host(live_u, live_logl, surv_idx, K, it, seed)
        else:
            cur, cur_logl = cur0, np.full(K, -5.0)
        point, inside, d = nested.propose_host(cur, live_u, surv_idx, q, seed, FGAMMA, P_UNIT,
                                               details=True)
        seen |= set(inside)
        calls.append(dict(live_u=live_u, live_logl=live_logl, surv_idx=surv_idx, nlive=nlive,
                          start=start, it=it, q=q, seed=seed, cur=cur, cur_logl=cur_logl,
                          point=point, inside=inside, a=d.a, b=d.b, gamma=d.gamma, prop=d.prop))
    assert seen == {0, 1}, (nfree, K, seen)
    return calls
