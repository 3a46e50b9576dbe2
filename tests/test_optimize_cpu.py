"""The optimiser's NumPy statements (pyratbay_amd/optimize.py, Retrieval.residuals_host), which
are the specification of csrc/pb_optimize.hip:

  * residuals_host against Observation.loglike_host + log_prior_host through
    -0.5 sum R^2 - 0.5 sum log(2 pi uncert^2) = log_posterior;
  * lm_host with an analytic Jacobian against scipy.optimize.least_squares and an exact solve,
    by bounds that are derived (optimize_cases.PARAMETER_GAP_FACTOR), never a bare parameter
    tolerance;
  * the finite-difference Jacobian against the analytic one within its truncation bound;
  * the damped Cholesky solve against a 50-digit solve (the yardstick of the device's bound).

lm_host's iteration counts (profiles/optimize.md): Rosenbrock 25, 12, 17, 34 (GTOL), bounded
Rosenbrock 14 (FTOL), the exponential fit 5, 8, 9 (FTOL)."""
import numpy as np
import pytest

import optimize_cases as oc
from pyratbay_amd import optimize as po

EPS = oc.EPS


# -------------------------------------------------------------------------------------------------
# the residual vector
# -------------------------------------------------------------------------------------------------
def residual_inputs(ret, nw, seed):
    """theta inside the bounds with the Gaussian priors hit on both sides, and model fluxes a few
    sigma off the data."""
    rng = np.random.default_rng(seed)
    f = ret.ifree
    theta = ret.params[f] + 3.0 * ret.pstep[f] * rng.uniform(-1, 1, (nw, ret.nfree))
    assert np.all(ret.inside_host(theta))
    model = ret.observation.data_host + rng.normal(0, 1.0, (nw, ret.observation.nbands))
    return theta, model


def test_residuals_give_the_log_posterior():
    ret = oc.cpu_retrieval()
    obs = ret.observation
    assert list(ret.igauss) == [0, 2] and ret.nfree == 4
    theta, model = residual_inputs(ret, 40, 1)
    ig = ret.igauss
    below = theta[:, ig] < ret.prior[ret.ifree][ig]
    assert below.any(axis=0).all() and (~below).any(axis=0).all()      # both sides of both priors
    R = ret.residuals_host(theta, model)
    assert R.shape == (40, obs.nbands + 2) and np.all(np.isfinite(R))
    split = ret.split_host(theta)
    assert np.ptp(split['offsets'][:, 0]) > 0 and np.all(split['offsets'][:, 1] == 3.0)
    assert np.all(split['err_pars'] == [0.2, 1.2])
    worst = 0.0
    for w in range(40):
        uncert = obs.scale_errors_host(split['err_pars'][w])
        assert np.all(uncert[[2, 3, 4, 5]] != obs.uncert_host[[2, 3, 4, 5]])
        chi2 = np.sum(R[w]**2)
        got = -0.5 * chi2 - 0.5 * np.sum(np.log(2.0 * np.pi * uncert**2.0))
        want = obs.loglike_host(model[w], split['offsets'][w], split['err_pars'][w]) + \
            ret.log_prior_host(theta[w:w + 1])[0]
        units = abs(got - want) / (EPS * chi2)
        worst = max(worst, units)
        assert units <= 4.0
    print(f'residual identity: worst {worst:.3f} units of eps sum R^2')


def test_residuals_reject_and_refuse():
    ret = oc.cpu_retrieval()
    theta, model = residual_inputs(ret, 4, 2)
    theta[1, 1] = -11.0                                     # below pmin
    theta[2, 0] = np.nan
    model[3, 4] = np.inf
    R = ret.residuals_host(theta, model)
    assert np.all(np.isfinite(R[0])) and np.all(R[1:] == np.inf)
    with pytest.raises(ValueError, match='model_host must have shape'):
        ret.residuals_host(theta, model[:, :3])
    free = oc.cpu_retrieval(free_errors=True)
    with pytest.raises(ValueError, match=r"\['err_scale_nrs2'\] are free"):
        free.residuals_host(np.tile(free.params[free.ifree], (1, 1)), model[:1])
    with pytest.raises(ValueError, match='are free'):
        free._check_least_squares()


# -------------------------------------------------------------------------------------------------
# lm_host against SciPy
# -------------------------------------------------------------------------------------------------
def check_against(name, st, ref_x, ref_cost, A_of, ftol=1e-10):
    """Every start: a status other than RUNNING and MAXIT under the cap, the cost gap within
    ftol max(cost, 1), the parameter gap D with 0.5 D^T A D within PARAMETER_GAP_FACTOR times that
    bound (A = J^T J at the reference's solution)."""
    for s in range(len(st.theta)):
        assert st.status[s] not in (po.RUNNING, po.MAXIT), (name, s, st.status[s])
        assert st.niter[s] < 100
        gap = oc.gap_bounds(st.cost[s], ref_cost[s], ftol)
        assert st.cost[s] - ref_cost[s] <= gap, (name, s, st.cost[s], ref_cost[s])
        D = st.theta[s] - ref_x[s]
        quad = 0.5 * D @ A_of(ref_x[s]) @ D
        assert quad <= oc.PARAMETER_GAP_FACTOR * gap, (name, s, quad, gap)
    print(f'{name}: iterations {list(st.niter)}, status '
          f'{[po.STATUS_NAMES[k] for k in st.status]}')


def scipy_fit(name, x0, **kw):
    from scipy.optimize import least_squares
    res, jac, *_ = oc.PROBLEMS[name]
    fit = least_squares(lambda x: res(x[None, :])[0], x0, jac=lambda x: jac(x[None, :])[0],
                        xtol=1e-14, ftol=1e-14, gtol=1e-14, **kw)
    return fit.x, fit.cost


def gauss_newton(name):
    jac = oc.PROBLEMS[name][1]

    def A_of(x):
        J = jac(x[None, :])[0]
        return J.T @ J
    return A_of


def test_linear_problem_in_one_iteration():
    lin = oc.linear_problem()
    x, *_ = np.linalg.lstsq(lin.M, lin.b, rcond=None)
    theta0 = np.random.default_rng(6).normal(0, 1, (3, 5))
    st = po.lm_host(lin.residuals, theta0, -100.0, 100.0, 1.0, jac=lin.jac, niter=1, lam0=1e-12)
    cost = 0.5 * np.sum((lin.M @ x - lin.b)**2)
    assert np.all(st.niter == 1) and np.all(st.picked == 0)
    A = lin.M.T @ lin.M
    for s in range(3):
        gap = oc.gap_bounds(st.cost[s], cost)
        D = st.theta[s] - x
        assert st.cost[s] - cost <= gap
        assert 0.5 * D @ A @ D <= oc.PARAMETER_GAP_FACTOR * gap


def test_rosenbrock():
    res, jac, pmin, pmax, scale, starts = oc.PROBLEMS['rosenbrock']
    st = po.lm_host(res, starts, pmin, pmax, scale, jac=jac)
    ref = [scipy_fit('rosenbrock', x0, method='lm') for x0 in starts]
    for x, cost in ref:
        assert np.allclose(x, [1.0, 1.0], atol=1e-12) and cost < 1e-24
    check_against('rosenbrock', st, [r[0] for r in ref], [r[1] for r in ref],
                  gauss_newton('rosenbrock'))


def test_bounded_rosenbrock():
    res, jac, pmin, pmax, scale, starts = oc.PROBLEMS['bounded']
    st = po.lm_host(res, starts, pmin, pmax, scale, jac=jac)
    x, cost = scipy_fit('bounded', starts[0], method='trf', bounds=(pmin, pmax))
    assert np.allclose(x, [0.5, 0.25], atol=1e-9) and abs(cost - 0.125) < 1e-12
    assert st.theta[0, 0] == 0.5                             # on the bound, exactly

    def A_of(xr):
        # the bound parameter is not part of the quadratic model: its gap is exact (above)
        A = gauss_newton('bounded')(xr)
        A[0, :] = A[:, 0] = 0.0
        return A
    check_against('bounded', st, [x], [cost], A_of)
    assert abs(st.cost[0] - 0.125) <= 1e-10


def test_exponential_fit():
    res, jac, pmin, pmax, scale, starts = oc.PROBLEMS['expfit']
    st = po.lm_host(res, starts, pmin, pmax, scale, jac=jac)
    ref = [scipy_fit('expfit', x0, method='lm') for x0 in starts]
    check_against('expfit', st, [r[0] for r in ref], [r[1] for r in ref], gauss_newton('expfit'))


def test_a_run_in_two_parts_and_refusals():
    res, jac, pmin, pmax, scale, starts = oc.PROBLEMS['expfit']
    whole = po.lm_host(res, starts, pmin, pmax, scale, niter=5)
    parts = po.lm_host(res, starts, pmin, pmax, scale, niter=2)
    parts = po.lm_host(res, starts, pmin, pmax, scale, niter=3, state=parts)
    for name in ('theta', 'cost', 'lam', 'status', 'niter'):
        assert np.array_equal(getattr(whole, name), getattr(parts, name))
    with pytest.raises(ValueError, match='outside the bounds'):
        po.lm_host(res, starts, pmin, 1.0, scale)
    with pytest.raises(ValueError, match=r'pmax - pmin < 2 h'):
        po.lm_host(res, starts, 0.0, 1e-4, scale)
    with pytest.raises(ValueError, match='unknown settings'):
        po.lm_host(res, starts, pmin, pmax, scale, lambda0=1.0)
    with pytest.raises(ValueError, match='129 free parameters'):
        po.check_problem(129, 0.0, 1.0, 1.0, 1e-4)
    # a start whose residual is not finite stalls at once, one with a zero gradient has GTOL
    st = po.lm_host(lambda t: np.where(t[:, :1] > 0.5, np.inf, t), np.array([[0.7, 0.1]]),
                    -1.0, 1.0, 1.0)
    assert st.status[0] == po.STALL and st.niter[0] == 0
    st = po.lm_host(lambda t: t * 1.0, np.zeros((1, 2)), -1.0, 1.0, 1.0)
    assert st.status[0] == po.GTOL and st.niter[0] == 0


# -------------------------------------------------------------------------------------------------
# finite differences
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fd_step', [1e-4, 1e-5])
def test_finite_difference_jacobian(fd_step):
    """|J_fd - J| <= h max|d2r/dtheta_k^2| / 2 (Taylor, the maximum over the step) plus the
    rounding of the two residuals, 4 eps (|a| e + |c| + |y|) each, over h."""
    theta = oc.FIT_STARTS.copy()
    theta[1, 1] = 10.0 - 0.5 * fd_step                      # a backward difference
    probe, step = po.probe_host(theta, np.full(3, 10.0), np.ones(3), fd_step)
    assert step[1, 1] == -fd_step and np.all(np.delete(step.ravel(), 4) == fd_step)
    assert np.array_equal(probe[:, 0], theta)
    R = oc.expfit(probe.reshape(-1, 3)).reshape(3, 4, -1)
    J_fd = (R[:, 1:] - R[:, :1]) / step[:, :, None]                         # [ns, nfree, m]
    J = np.swapaxes(oc.expfit_jac(theta), 1, 2)
    k = np.arange(3)
    moved = probe[:, k + 1, :]                                              # [ns, k, nfree]
    second = np.maximum(oc.expfit_second(theta),
                        np.stack([oc.expfit_second(moved[:, j])[:, j] for j in k], axis=1))
    mag = np.abs(theta[:, :1]) * np.exp(np.abs(theta[:, 1:2]) * 2.0 + fd_step) + \
        np.abs(theta[:, 2:]) + np.max(np.abs(oc.FIT_Y)) + fd_step
    bound = 0.5 * fd_step * second + 2 * 4 * EPS * mag / fd_step
    err = np.max(np.abs(J_fd - J), axis=2)
    assert np.all(err <= bound), (err, bound)
    assert np.all(err[:, 1] > 0)
    # and the normal equations are those of that Jacobian
    A, g, cost = po.normal_host(R, step)
    assert np.allclose(A, np.einsum('ski,sli->skl', J_fd, J_fd), rtol=1e-12, atol=0)
    assert np.array_equal(A, np.swapaxes(A, 1, 2))
    assert np.allclose(g, np.einsum('ski,si->sk', J_fd, R[:, 0]), rtol=1e-9)
    assert np.allclose(cost, 0.5 * np.sum(R[:, 0]**2, axis=1), rtol=1e-14)


def test_finite_difference_run_against_the_analytic_run():
    res, jac, pmin, pmax, scale, starts = oc.PROBLEMS['expfit']
    exact = po.lm_host(res, starts, pmin, pmax, scale, jac=jac)
    fd = po.lm_host(res, starts, pmin, pmax, scale, fd_step=1e-5)
    check_against('expfit, finite differences', fd, exact.theta, exact.cost,
                  gauss_newton('expfit'))
    print('largest parameter difference', np.max(np.abs(fd.theta - exact.theta)))


def test_frozen_column_and_cost_order():
    R, step = oc.normal_case(5, 130, 2, 3)
    A, g, cost = po.normal_host(R, step)
    assert np.all(A[1, 4, :] == 0) and np.all(A[1, :, 4] == 0) and g[1, 4] == 0
    assert np.all(np.isfinite(A)) and np.all(np.diagonal(A[0]) > 0) and np.all(A[1, :4, :4] != 0)
    assert np.array_equal(A, np.swapaxes(A, 1, 2))
    # cost_host: 64 lane-strided sums, then the butterfly
    r = R[0, 0]
    lanes = [sum(r[j::64]**2, 0.0) for j in range(64)]
    while len(lanes) > 1:
        h = len(lanes) // 2
        lanes = [lanes[i] + lanes[i + h] for i in range(h)]
    assert abs(cost[0] - 0.5 * lanes[0]) <= 64 * EPS * cost[0]
    assert po.cost_host(np.array([3.0, np.inf])) == np.inf


# -------------------------------------------------------------------------------------------------
# the damped solve against 50 digits
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nfree', oc.SOLVE_NFREES)
def test_damped_solve_against_mpmath(nfree):
    """The error of the step in units of cond eps, cond the condition number of the damped system
    in its diagonal scaling; asserted below n (3 n + 1), Cholesky's backward error bound
    (Higham, Accuracy and Stability, theorem 10.4, with || |L| |L^T| || <= n ||A||)."""
    worst = 0.0
    for cond in oc.SOLVE_CONDS:
        c = oc.solve_case(nfree, cond)
        lam = np.full(1, oc.SOLVE_LAM)
        trial, pgrad = po.step_host(c.A[None], c.g[None], c.theta[None], lam, c.pmin, c.pmax,
                                    c.scale, oc.SOLVE_NU, oc.SOLVE_NTRIAL)
        assert np.all(np.isfinite(trial))
        active = po.active_host(c.A, c.g, c.theta, c.pmin, c.pmax)
        if nfree > 2:
            assert active[1] and active[2] and (nfree == 3 or not active[3])
        assert np.array_equal(trial[0][:, active], np.tile(c.theta[active], (4, 1)))
        for j in range(oc.SOLVE_NTRIAL):
            lj = po.trial_lambda(oc.SOLVE_LAM, oc.SOLVE_NU, j)
            f, exact, kappa = oc.solve_exact(nfree, cond, j)
            assert np.array_equal(f, np.where(~active)[0])
            if nfree <= 17 or (cond == 1e8 and j == 0):
                # the fixture against the 50-digit solve it was made by (all of it takes a minute)
                f2, exact2, kappa2 = oc.solve_exact_mpmath(c, lj)
                assert np.array_equal(f, f2) and np.array_equal(exact, exact2)
                assert abs(kappa / kappa2 - 1) < 1e-6
            # the solve itself
            Af = c.A[np.ix_(f, f)]
            M = Af.copy()
            np.fill_diagonal(M, np.diag(Af) + lj * np.diag(Af))
            L = po.cholesky_host(M)
            delta = po.cholesky_solve_host(L, -c.g[f])
            units = oc.solve_error(c, f, delta, exact) / (kappa * EPS)
            worst = max(worst, units)
            assert units <= nfree * (3 * nfree + 1)
            # the trial point: clipped exactly
            want = np.minimum(np.maximum(c.theta[f] + delta, c.pmin[f]), c.pmax[f])
            assert np.array_equal(trial[0, j, f], want)
            assert np.all((trial[0, j] >= c.pmin) & (trial[0, j] <= c.pmax))
            if nfree > 3 and delta[list(f).index(3)] > 0:
                assert trial[0, j, 3] == 0.0                   # clipped to pmax
        free = ~active
        assert pgrad[0] == np.max(np.abs(c.g[free]) * c.scale[free])
    print(f'damped solve nfree {nfree}: worst {worst:.3f} units of cond eps')


def test_failed_pivot_and_covariance():
    A = np.array([[1.0, 2.0], [2.0, 1.0]])                   # indefinite
    g, theta = np.array([0.3, -0.2]), np.zeros(2)
    lo, hi, scale = np.full(2, -1.0), np.full(2, 1.0), np.ones(2)
    trial, _ = po.step_host(A[None], g[None], theta[None], np.full(1, 1e-3), lo, hi, scale)
    assert np.array_equal(trial, np.zeros((1, 4, 2)))
    C, active, singular = po.covariance_host(A[None], g[None], theta[None], lo, hi)
    assert singular[0] == 1 and np.all(np.isnan(C)) and not active.any()
    c = oc.solve_case(17, 1e4)
    C, active, singular = po.covariance_host(c.A[None], c.g[None], c.theta[None], c.pmin, c.pmax)
    f = np.where(active[0] == 0)[0]
    assert singular[0] == 0 and list(np.where(active[0])[0]) == [1, 2]
    assert np.all(C[0][active[0] == 1] == 0) and np.all(C[0][:, active[0] == 1] == 0)
    assert np.array_equal(C[0], C[0].T)
    resid = C[0][np.ix_(f, f)] @ c.A[np.ix_(f, f)] - np.eye(len(f))
    w = np.sqrt(np.diag(c.A)[f])
    kappa = np.linalg.cond(c.A[np.ix_(f, f)] / w[:, None] / w[None, :])
    # (in the diagonal scaling: W C A W^-1 - I)
    assert np.max(np.abs(resid * w[:, None] / w[None, :])) <= 17 * 52 * kappa * EPS
