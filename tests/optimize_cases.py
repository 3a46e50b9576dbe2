"""Cases the optimiser's CPU and GPU tests share (pyratbay_amd/optimize.py, csrc/pb_optimize.hip):
the least-squares problems lm_host is tested on against SciPy, written once for NumPy and torch;
the matrices of the damped-solve tests with their 50-digit solutions; inputs of the kernels; and
the small emission retrieval of sampler_cases restated with fixed error parameters."""
import functools
import os
import types

import numpy as np

EPS = np.finfo(float).eps


# -------------------------------------------------------------------------------------------------
# least-squares problems: residuals(xp) works on NumPy arrays or torch tensors theta[n, nfree]
# -------------------------------------------------------------------------------------------------
def _stack(cols):
    if isinstance(cols[0], np.ndarray):
        return np.stack(cols, axis=1)
    import torch
    return torch.stack(cols, dim=1)


def _const(a, like):
    if isinstance(like, np.ndarray):
        return np.asarray(a, dtype=np.float64)
    import torch
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=like.device)


def _exp(x):
    if isinstance(x, np.ndarray):
        return np.exp(x)
    import torch
    return torch.exp(x)


def rosenbrock(theta):
    x, y = theta[:, 0], theta[:, 1]
    return _stack([10.0 * (y - x * x), 1.0 - x])


def rosenbrock_jac(theta):
    x = theta[:, 0]
    J = np.zeros((len(theta), 2, 2))
    J[:, 0, 0], J[:, 0, 1], J[:, 1, 0] = -20.0 * x, 10.0, -1.0
    return J


ROSENBROCK_STARTS = np.array([[-1.2, 1.0], [3.0, -3.0], [0.0, 0.0], [-2.0, 4.0]])

# a * exp(b t) + c, m = 50, noise 0.02, seed 3
FIT_T = np.linspace(0.0, 2.0, 50)
FIT_TRUE = np.array([1.5, -1.3, 0.4])
FIT_Y = FIT_TRUE[0] * np.exp(FIT_TRUE[1] * FIT_T) + FIT_TRUE[2] + \
    np.random.default_rng(3).normal(0.0, 0.02, 50)
FIT_STARTS = np.array([[1.0, -1.0, 0.0], [3.0, -0.2, 1.0], [0.5, -3.0, -0.5]])


def expfit(theta):
    t, y = _const(FIT_T, theta), _const(FIT_Y, theta)
    a, b, c = theta[:, 0:1], theta[:, 1:2], theta[:, 2:3]
    return a * _exp(b * t[None, :]) + c - y[None, :]


def expfit_jac(theta):
    a, b = theta[:, 0:1], theta[:, 1:2]
    e = np.exp(b * FIT_T[None, :])
    return np.stack([e, a * FIT_T[None, :] * e, np.ones_like(e)], axis=2)


def expfit_second(theta):
    """max_i |d2 r_i / d theta_k^2| per parameter, [n, 3]: 0, a t^2 exp(b t), 0."""
    a, b = theta[:, 0:1], theta[:, 1:2]
    d2b = np.max(np.abs(a * FIT_T[None, :]**2 * np.exp(b * FIT_T[None, :])), axis=1)
    return np.stack([np.zeros_like(d2b), d2b, np.zeros_like(d2b)], axis=1)


def linear_problem(seed=5, m=20, n=5):
    rng = np.random.default_rng(seed)
    M, b = rng.normal(0, 1, (m, n)), rng.normal(0, 1, m)

    def residuals(theta):
        return theta @ _const(M, theta).T - _const(b, theta)[None, :]

    def jac(theta):
        return np.repeat(M[None, :, :], len(theta), axis=0)
    return types.SimpleNamespace(M=M, b=b, residuals=residuals, jac=jac)


PROBLEMS = {
    # name: (residuals, jac, pmin, pmax, scale, starts)
    'rosenbrock': (rosenbrock, rosenbrock_jac, -10.0, 10.0, 1.0, ROSENBROCK_STARTS),
    'bounded': (rosenbrock, rosenbrock_jac, np.array([-10.0, -10.0]), np.array([0.5, 10.0]), 1.0,
                ROSENBROCK_STARTS[:1]),
    'expfit': (expfit, expfit_jac, -10.0, 10.0, 1.0, FIT_STARTS),
}


def gap_bounds(st_cost, ref_cost, ftol=1e-10):
    """The bound on a cost gap between two converged runs, ftol max(cost, 1)."""
    return ftol * np.maximum(np.maximum(st_cost, ref_cost), 1.0)


# The factor of the parameter bound.  Both runs end within gap = ftol max(cost, 1) of the
# minimum's cost (FTOL's own criterion, one further step would gain less), and near a minimum
# cost(x) - cost* = 0.5 (x - x*)^T A (x - x*) to second order: so each end lies in the ellipsoid
# 0.5 d^T A d <= gap, and two points of it are at most 0.5 D^T A D <= (sqrt(gap) + sqrt(gap))^2 = 4
# gap apart (triangle inequality in the A-norm).  Twice that for the second-order remainder.
PARAMETER_GAP_FACTOR = 8.0


# -------------------------------------------------------------------------------------------------
# the damped solves
# -------------------------------------------------------------------------------------------------
SOLVE_NFREES = (1, 2, 17, 128)
SOLVE_CONDS = (1e0, 1e4, 1e8)
SOLVE_LAM, SOLVE_NU, SOLVE_NTRIAL = 1e-3, 10.0, 4


def solve_bounds(nfree):
    """pmin, pmax of the solve cases: -1 .. 1, but 0 .. 2 for parameter 2 and -2 .. 0 for parameter
    3, which sit at 0 like the others: on their lower and upper bound."""
    pmin, pmax = np.full(nfree, -1.0), np.full(nfree, 1.0)
    if nfree > 2:
        pmin[2], pmax[2] = 0.0, 2.0
    if nfree > 3:
        pmin[3], pmax[3] = -2.0, 0.0
    return pmin, pmax


def make_solve_case(nfree, cond, seed=0):
    """(What the fixture's cases were made by.)  A[nfree, nfree] symmetric positive definite on
    its free part with condition number about `cond` AFTER the diagonal scaling LM's damping works
    in (a random orthogonal basis, log-spaced eigenvalues, then row and column scales over four
    decades), one zero-diagonal column (column 1 where nfree > 2), g, and theta = 0: a trial point
    is then the step itself, with no rounding of theta + delta between the solve and its
    measurement.  Where nfree allows, parameter 2 is on its lower bound and pushed outward
    (active), parameter 3 on its upper bound and pushed inward (free; a positive step is clipped)."""
    rng = np.random.default_rng(1000 * nfree + int(np.log10(cond)) + seed)
    Q, _ = np.linalg.qr(rng.normal(0, 1, (nfree, nfree)))
    ev = np.logspace(0, -np.log10(cond), nfree) if nfree > 1 else np.ones(1)
    core = (Q * ev) @ Q.T
    core = 0.5 * (core + core.T)
    d = 10.0**rng.uniform(-2, 2, nfree)
    A = core * d[:, None] * d[None, :]
    g = rng.normal(0, 1, nfree) * d
    theta = np.zeros(nfree)
    pmin, pmax = solve_bounds(nfree)
    if nfree > 2:
        A[1, :] = 0.0
        A[:, 1] = 0.0
        g[2] = abs(g[2]) + 0.1                          # on pmin, pushed outward: active
    if nfree > 3:
        g[3] = abs(g[3]) + 0.1                          # on pmax, pushed inward: free
    # g scaled (the active set depends on its signs alone) so that the largest step of the
    # weakest damping is 0.4: the interior parameters stay inside, and clipping is met only at
    # the parameter that starts on pmax
    from pyratbay_amd import optimize
    f = np.where(~optimize.active_host(A, g, theta, pmin, pmax))[0]
    Af = A[np.ix_(f, f)]
    delta = np.linalg.solve(Af + SOLVE_LAM / SOLVE_NU * np.diag(np.diag(Af)), -g[f])
    g = g * (0.4 / np.max(np.abs(delta)))
    return types.SimpleNamespace(A=A, g=g, theta=theta, pmin=pmin, pmax=pmax,
                                 scale=np.full(nfree, 0.1), nfree=nfree, cond=cond)


SOLVE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                            'g30_optimize_solve.npz')


@functools.lru_cache(maxsize=None)
def solve_case(nfree, cond):
    """make_solve_case's result as the fixture holds it (A, g and theta are stored, not made
    again: another machine's linear algebra library would round the matrix differently, and
    the 50-digit solutions belong to these bits).  Do not modify the result."""
    g = _solve_golden()
    key = f'n{nfree}_c{int(np.log10(cond))}'
    pmin, pmax = solve_bounds(nfree)
    return types.SimpleNamespace(A=g[key + '_A'], g=g[key + '_g'], theta=g[key + '_theta'],
                                 pmin=pmin, pmax=pmax, scale=np.full(nfree, 0.1), nfree=nfree,
                                 cond=cond)


def trial_lam(j):
    from pyratbay_amd import optimize
    return optimize.trial_lambda(SOLVE_LAM, SOLVE_NU, j)


@functools.lru_cache(maxsize=None)
def _solve_golden():
    return dict(np.load(SOLVE_GOLDEN))


def solve_exact(nfree, cond, j):
    """(free indices, delta at 50 digits rounded to double, the condition number of the damped
    free system in its diagonal scaling) of solve_case at trial j's damping, from the fixture
    g30_optimize_solve.npz: solve_exact_mpmath's results, which take a minute to compute
    (`python tests/optimize_cases.py` writes the file; test_optimize_cpu recomputes a part)."""
    g = _solve_golden()
    key = f'n{nfree}_c{int(np.log10(cond))}_j{j}'
    return g[key + '_free'], g[key + '_delta'], float(g[key + '_kappa'])


def write_solve_golden():
    out = {}
    for nfree in SOLVE_NFREES:
        for cond in SOLVE_CONDS:
            c = make_solve_case(nfree, cond)
            key = f'n{nfree}_c{int(np.log10(cond))}'
            out[key + '_A'], out[key + '_g'], out[key + '_theta'] = c.A, c.g, c.theta
            for j in range(SOLVE_NTRIAL):
                f, delta, kappa = solve_exact_mpmath(c, trial_lam(j))
                key = f'n{nfree}_c{int(np.log10(cond))}_j{j}'
                out[key + '_free'], out[key + '_delta'], out[key + '_kappa'] = f, delta, kappa
    np.savez_compressed(SOLVE_GOLDEN, **out)


def solve_exact_mpmath(c, lam):
    """solve_exact, computed for the case c: a 50-digit LU solve of the damped free system."""
    import mpmath
    from pyratbay_amd import optimize
    f = np.where(~optimize.active_host(c.A, c.g, c.theta, c.pmin, c.pmax))[0]
    Af = c.A[np.ix_(f, f)]
    with mpmath.workdps(50):
        M = mpmath.matrix(Af.tolist())
        for a in range(len(f)):
            M[a, a] = M[a, a] * (1 + mpmath.mpf(lam))
        x = mpmath.lu_solve(M, mpmath.matrix((-c.g[f]).tolist()))
        delta = np.array([float(v) for v in x])
    Md = Af + lam * np.diag(np.diag(Af))
    s = 1.0 / np.sqrt(np.diag(Md))
    return f, delta, float(np.linalg.cond(Md * s[:, None] * s[None, :]))


def solve_error(c, f, delta, exact):
    """The error of a step in the norm the bound is stated in: the scaled variables
    z = sqrt(diag) delta of the equilibrated system, relative, 2-norm."""
    w = np.sqrt(np.diag(c.A)[f])
    return float(np.linalg.norm(w * (delta - exact)) / np.linalg.norm(w * exact))


# -------------------------------------------------------------------------------------------------
# inputs of pb_lm_normal
# -------------------------------------------------------------------------------------------------
NORMAL_MS = (1, 2, 63, 64, 65, 257, 4099)       # PB_LM_CHUNK = 64: below, at, above; many chunks
NORMAL_NFREES = (1, 2, 15, 16, 17, 64, 128)     # the 2 x 2 thread tile and the 32 x 32 block tile
NORMAL_NS = (1, 5)


def normal_case(nfree, m, ns, seed):
    """R[ns, nfree + 1, m] and step[ns, nfree]: a smooth residual plus differences of the size
    h J with Jacobian columns over four decades; every third column a backward difference; the
    last column of the last start frozen by a +inf probe residual."""
    rng = np.random.default_rng(seed)
    h = 1e-4 * 10.0**rng.uniform(-2, 2, nfree)
    step = np.tile(h, (ns, 1))
    step[:, ::3] *= -1.0
    J = rng.normal(0, 1, (ns, nfree, m)) * 10.0**rng.uniform(-2, 2, (1, nfree, 1))
    R0 = rng.normal(0, 1, (ns, 1, m))
    R = np.concatenate((R0, R0 + J * step[:, :, None]), axis=1)
    R[ns - 1, nfree, m // 2] = np.inf
    return R, step


# -------------------------------------------------------------------------------------------------
# the retrieval
# -------------------------------------------------------------------------------------------------
CPU_BLOCK = """
    T_irr          1400.0   100.0  3000.0   50.0  1500.0  100.0  200.0
    log_H2O          -3.5   -10.0    -1.0    0.3
    R_planet          1.0     0.5     2.0    0.05    1.1    0.2
    log_k_ray         0.5    -5.0     5.0   -2
    offset_nrs1      10.0  -100.0   100.0    5.0
    offset_miri       3.0  -100.0   100.0    0.0
    err_scale_nrs2    0.2    -1.0     1.0    {estep}
    err_quad_miri     1.2    -3.0     3.0    0.0
    T_eff          5500.0
"""
CPU_BANDS = ['nrs1 a', 'nrs1 b', 'nrs2 a', 'nrs2 b', 'miri a', 'miri b', 'other']


def cpu_retrieval(free_errors=False):
    """A Retrieval on stand-ins (test_retrieval_cpu's), for the host statements: seven data
    points, two offsets (one free), error models of both kinds (fixed unless free_errors), a
    two-sided and a symmetric Gaussian prior, a shared and a fixed line."""
    import test_retrieval_cpu as trc
    from pyratbay_amd import observation as po
    from pyratbay_amd import retrieval as pr
    base = np.array([-1.5, -0.8, 0.2, 0.4, 1400.0, 150.0, -3.4, 7.5e9])
    atm = trc.atmosphere(['rplanet'], base_params=base)
    model, _ = trc.stand_ins(cont=trc.continuum())
    bands = types.SimpleNamespace(nbands=len(CPU_BANDS), star_grid=object())
    rng = np.random.default_rng(21)
    obs = po.Observation(rng.uniform(1.0, 2.0, 7), rng.uniform(0.1, 0.5, 7), CPU_BANDS,
                         ['offset_nrs1', 'offset_miri'], ['err_scale_nrs2', 'err_quad_miri'],
                         units='percent')
    return pr.Retrieval(model, atm, bands, obs,
                        CPU_BLOCK.format(estep=0.1 if free_errors else 0.0))


OPT_STARTS = 8


def emission_retrieval(eng, golden, free_errors=False):
    """sampler_cases.emission_retrieval with its two err_* lines fixed (free_errors: as they
    are)."""
    import sampler_cases as sc
    ret = sc.emission_retrieval(eng, golden)
    if free_errors:
        return ret
    block = '\n'.join('  '.join([name] + [repr(float(v)) for v in row]) for name, row in zip(
        ret.pnames, zip(ret.params, ret.pmin, ret.pmax,
                        np.where([n.startswith('err_') for n in ret.pnames], 0.0, ret.pstep),
                        ret.prior, ret.priorlow, ret.priorup)))
    return eng.Retrieval(ret.model, ret.atmosphere, ret.bands, ret.observation, block, chunk=2)


def emission_starts(ret, seed=4):
    """theta0[8, nfree] within one pstep of the block's values: inside the bounds."""
    rng = np.random.default_rng(seed)
    f = ret.ifree
    theta0 = ret.params[f] + ret.pstep[f] * rng.uniform(-1, 1, (OPT_STARTS, ret.nfree))
    assert np.all(ret.inside_host(theta0))
    return theta0


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_solve_golden()
