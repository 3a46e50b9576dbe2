"""Cases the sampler's CPU and GPU tests share (pyratbay_amd/sampler.py, csrc/pb_sampler.hip):
the published Philox known answers, the Gaussian target the statements are tested on with its
committed statistical bounds, inputs for the propose and accept kernels, and the small emission
retrieval of tests/test_gpu_retrieval.py restated for Retrieval.sample."""
import functools

import numpy as np

EPS = np.finfo(float).eps

# Random123's known answers of philox4x32-10: (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# -------------------------------------------------------------------------------------------------
# the Gaussian target
# -------------------------------------------------------------------------------------------------
MU = np.array([1.0, -2.0, 0.5])
SIGMA = np.array([0.5, 2.0, 0.1])
RHO = 0.8                                   # between the first two
CORR = np.array([[1.0, RHO, 0.0], [RHO, 1.0, 0.0], [0.0, 0.0, 1.0]])
NCHAINS, NGEN, BURN = 16, 3000, 500
RUN_KW = dict(pstep=0.1 * SIGMA, fepsilon=0.01)

# The worst values of run_host over seeds 0 - 19 (profiles/sampler.md has the table), and the
# committed bounds: twice each, because 20 seeds sample the tail thinly.
WORST_MEAN, WORST_STD, WORST_CORR = 0.04552, 0.02770, 0.02614
BOUND_MEAN, BOUND_STD, BOUND_CORR = 2 * WORST_MEAN, 2 * WORST_STD, 2 * WORST_CORR
ACCEPTANCE = (0.2, 0.35)                    # (measured over those seeds: 0.263 - 0.278)


def _quadratic(a, b, c):
    return -0.5 * ((a * a - (2.0 * RHO) * (a * b) + b * b) / (1.0 - RHO * RHO) + c * c)


def log_post_host(theta):
    """[nw]: the Gaussian's log-density (no normalisation), -inf outside MU +- 10 SIGMA."""
    t = (np.asarray(theta) - MU) / SIGMA
    with np.errstate(invalid='ignore'):
        inside = np.all(np.abs(t) <= 10.0, axis=1)
    return np.where(inside, _quadratic(t[:, 0], t[:, 1], t[:, 2]), -np.inf)


def log_post_torch():
    """The same operations as a torch callable on device tensors."""
    import torch
    mu = torch.as_tensor(MU, device='cuda')
    sigma = torch.as_tensor(SIGMA, device='cuda')

    def log_post(theta):
        t = (theta - mu) / sigma
        inside = torch.all(torch.abs(t) <= 10.0, dim=1)
        return torch.where(inside, _quadratic(t[:, 0], t[:, 1], t[:, 2]),
                           torch.full_like(t[:, 0], -float('inf')))
    return log_post


def gaussian_start(seed):
    """z0[160, 3] = MU + 3 SIGMA U(-1, 1) (NumPy's generator: inputs, not part of the sampler);
    the starting states are its last 16 rows."""
    rng = np.random.default_rng(1000 + seed)
    z0 = MU + 3.0 * SIGMA * rng.uniform(-1.0, 1.0, (10 * NCHAINS, 3))
    return z0[-NCHAINS:].copy(), z0


@functools.lru_cache(maxsize=None)
def gaussian_run_host(seed, ngen):
    """run_host on the target (computed once per session; do not modify the result)."""
    from pyratbay_amd import sampler
    theta0, z0 = gaussian_start(seed)
    return sampler.run_host(log_post_host, theta0, z0, ngen, seed=seed, **RUN_KW)


def statistics(theta, counts):
    """(worst |mean - MU| / SIGMA, worst relative error of the standard deviation, worst error of
    a correlation coefficient) of weighted samples."""
    w = counts / np.sum(counts)
    mean = np.sum(w[:, None] * theta, axis=0)
    dev = theta - mean
    cov = (w[:, None] * dev).T @ dev
    std = np.sqrt(np.diag(cov))
    corr = cov / np.outer(std, std)
    return (float(np.max(np.abs(mean - MU) / SIGMA)), float(np.max(np.abs(std / SIGMA - 1.0))),
            float(np.max(np.abs(corr - CORR))))


# -------------------------------------------------------------------------------------------------
# inputs of the kernels
# -------------------------------------------------------------------------------------------------
P_SNOOKER = 0.5
FGAMMA, FEPSILON = 0.9, 0.05
NFREES, NWS, MS = (1, 2, 63, 64, 65, 128), (1, 5, 65), (3, 1000)


def propose_case(nfree, nw, M, seed):
    """theta[nw, nfree], z[M + 2, nfree] (two NaN rows behind the history: nothing may read
    them), pstep[nfree], and a generation to start from.  Normal draws with parameter-dependent
    scales over four decades."""
    rng = np.random.default_rng(seed)
    scale = 10.0**rng.uniform(-2, 2, nfree)
    theta = scale * rng.normal(0, 1, (nw, nfree))
    z = np.full((M + 2, nfree), np.nan)
    z[:M] = scale * rng.normal(0, 1, (M, nfree))
    pstep = 0.1 * scale
    g = int(rng.integers(1, 2**31))
    return theta, z, pstep, g


def accept_case(nfree, nw, cap, seed):
    """A state (sampler.new_state_host) of nw chains with a store of cap rows each and a history
    of 4 rows."""
    from pyratbay_amd import sampler
    rng = np.random.default_rng(seed)
    theta = rng.normal(0, 1, (nw, nfree)) * 10.0**rng.uniform(-1, 1, nfree)
    logp = rng.uniform(-50.0, -1.0, nw)
    z0 = rng.normal(0, 1, (4, nfree))
    return sampler.new_state_host(theta, logp, z0, cap, thin_z=1)


def accept_inputs(st, g, seed, rng):
    """prop, logp_prop, log_jac for one call on the state st: differences of order one around the
    accept threshold (a good third of the chains accept), special values every fourth generation,
    and every finite margin |ln u - (delta + log_jac)| exceeds 1e-9 (asserted)."""
    from pyratbay_amd import sampler
    nw, nfree = st.theta.shape
    prop = st.theta + rng.normal(0, 0.3, (nw, nfree))
    log_jac = np.where(rng.uniform(0, 1, nw) < 0.5, 0.0, rng.normal(0, 0.5, nw))
    logp_prop = st.logp + rng.normal(-0.7, 1.5, nw)
    if g % 4 == 0:
        # chains 1 - 4 in turn: a NaN proposal, a -inf proposal, a NaN log_jac and, now and then
        # (a chain at +inf accepts nothing any more), a +inf proposal
        for k, w in enumerate(range(1, min(nw, 5))):
            what = (k + g // 4) % 4
            if what == 2:
                log_jac[w] = np.nan
            elif what < 2:
                logp_prop[w] = (np.nan, -np.inf)[what]
            elif g % 16 == 0:
                logp_prop[w] = np.inf
    margin = sampler.accept_margin_host(st.logp, logp_prop, log_jac, g, seed)
    finite = np.isfinite(margin)
    assert np.all(np.abs(margin[finite]) > 1e-9)
    return prop, logp_prop, log_jac


# -------------------------------------------------------------------------------------------------
# the small emission retrieval (tests/test_gpu_retrieval.py, e2e_case('emission'), restated)
# -------------------------------------------------------------------------------------------------
EMISSION_BLOCK = """
    log_kappa'    -1.5    -3.0     1.0    0.1
    log_gamma1    -0.8    -3.0     1.0    0.1
    log_gamma2     0.2    -2.0     2.0    0.0
    alpha          0.4
    T_irr       1400.0     0.0  3000.0   50.0  1450.0   100.0   200.0
    T_int        150.0     0.0   500.0   10.0
    log_H2O       -3.4    -9.0    -1.0    0.2
    log_CO        -3.3    -9.0    -1.0   -7
    log_Na         0.0    -2.0     2.0    0.1
    R_planet      1.05     0.5     2.0    0.02
    T_eff       5200.0  4000.0  6500.0   50.0  5300.0   200.0
    offset_nrs1    0.0  {omin}  {omax}    1.0
    offset_miri    0.0  {omin}  {omax}    1.0
    err_scale_nrs2 0.0    -1.0     1.0    0.1
    err_quad_miri  {q}    {qmin}  {qmax}  0.1
"""
E2E_CHAINS, E2E_NGEN = 8, 30


def emission_retrieval(eng, golden):
    """The Retrieval of test_gpu_retrieval's emission case: three bands, an eclipse with a free
    stellar temperature, two offsets and two error models, 11 free parameters, chunks of 2."""
    import test_gpu_atmosphere as atm_setup
    import test_gpu_batch_continuum as base
    from pyratbay_amd import atmosphere as pa
    s = atm_setup.spectrum_case(eng, pa, golden('g7_continuum'), 5, 77, False, False)
    wn, atm = s['wn'], s['atm']
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, s['base_radius'], 8.8e10,
                              rt_path='emission', column_order=None, continuum=s['cont'])
    bands, _ = base.make_bands(eng, wn)
    pb = eng.PassBands(wn, bands)
    sed_temps = np.array([4000.0, 5000.0, 6500.0])
    x = np.linspace(0.0, 1.0, len(wn))
    fluxes = 2.0e5 * (sed_temps[:, None] / 5000.0)**3 * (1 + 0.2 * np.sin(7 * x)[None, :])
    pb.set_eclipse_grid(8.8e10, eng.StellarGrid(wn, sed_temps, fluxes))
    flux = model.eval_params(atm, eng.dev(atm.base_params[None, :]), pb,
                             tstar=eng.dev(np.full(1, 5200.0))).cpu().numpy()[0]
    assert np.all(np.isfinite(flux)) and np.all(flux > 0)
    rng = np.random.default_rng(11)
    data = flux * (1 + rng.normal(0, 0.02, 3))
    obs = eng.Observation(data, 0.03 * flux, ['nrs1', 'nrs2', 'miri'],
                          ['offset_nrs1', 'offset_miri'], ['err_scale_nrs2', 'err_quad_miri'],
                          units='ppm')
    top = np.max(flux) * 1e4
    q = np.log10(np.max(flux) * 1e6 * 0.03)
    block = EMISSION_BLOCK.format(omin=-top, omax=top, q=q, qmin=q - 1, qmax=q + 1)
    return eng.Retrieval(model, atm, pb, obs, block, chunk=2)


def emission_history(ret, seed):
    """z0[80, nfree] around the block's values, within one pstep: inside the bounds."""
    rng = np.random.default_rng(seed)
    f = ret.ifree
    z0 = ret.params[f] + ret.pstep[f] * rng.uniform(-1, 1, (10 * E2E_CHAINS, ret.nfree))
    assert np.all(ret.inside_host(z0))
    return z0
