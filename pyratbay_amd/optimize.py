"""Batched multi-start Levenberg-Marquardt for the retrieval loop: the maximum of the posterior
(the reference's `bestp`, which mc3's least-squares fit ahead of the chains provides) and its
Laplace covariance, for many starts at once with launches only.  The finite-difference Jacobian
is made for the batched engine: the nfree + 1 probe points of every start are one walker batch,
the ntrial damping trials of every start another, so one iteration is two residual calls and a
few small kernels (csrc/pb_optimize.hip).  The NumPy statements here (probe_host, cost_host,
normal_host, active_host, cholesky_host, step_host, update_host, covariance_host, lm_host) ARE the
specification; where the issue text that asked for this module and lm_host differ in a detail,
lm_host decides.  Those details:

  * a start whose own residual is not finite (cost = +inf: outside the bounds, or a rejected
    model) ends with STALL at once: there is nothing to difference;
  * GTOL is looked at before the step of an iteration, on the gradient at the current point, and
    does not count as an iteration;
  * a trial whose step comes out non-finite is a failure like a bad pivot: trial = theta;
  * the finite difference uses the nominal step h_k, not fl(theta_k + h_k) - theta_k;
  * STALL is also how a start ends that sits at a minimum to rounding: no trial is strictly
    below the cost any more, every iteration is a reject and lam passes lam_max after a few.
    Such a start is at its optimum; a STALL far from one shows in its cost;
  * lam never falls below lam_min (1e-15), which the issue's defaults do not name;
  * the covariance calls A_ff singular when it is numerically so: a pivot that is not above
    nf eps A_pp (covariance_host).  With the bare test `pivot <= 0` an underdetermined J^T J
    would pass or fail by the sign of a rounding error.

One iteration, for ns starts at once:

    probe    [ns, nfree + 1, nfree]: row 0 = theta; row k + 1 = theta + hs_k e_k, hs_k = +h_k, or
             -h_k where theta_k + h_k > pmax_k; h_k = fd_step scale_k.
    normal   R = residuals(probe) [ns, nfree + 1, m]; D_ik = R[k+1, i] - R[0, i];
                 A_kl = (sum_i D_ik D_il / hs_min(k,l)) / hs_max(k,l),  g_k = (sum_i D_ik R0_i) / hs_k
             summed over i in index order, products and sums rounded separately;
             cost = 0.5 |R0|^2 in cost_host's order.  A column with a non-finite difference is
             frozen for this iteration: its row and column of A and its g are 0.
    step     active: (theta_k <= pmin_k and g_k > 0) or (theta_k >= pmax_k and g_k < 0) or
             A_kk == 0.  On the rest f: (A_ff + lam_j diag(A_ff)) delta = -g_f by Cholesky for
             lam_j = lam nu^(j-1), j = 0 .. ntrial - 1; trial_j = clip(theta + delta, pmin, pmax);
             a pivot <= 0 or not finite: trial_j = theta.  pgrad = max_f |g_k| scale_k.
    update   Rt = residuals(trial) [ns, ntrial, m]; the lowest finite trial cost wins, ties to the
             lowest index.  Below cost: accepted, lam = max(lam_j / nu, lam_min); else
             lam = lam nu^ntrial.  Status (update_host).

The defaults (fd_step 1e-4, ntrial 4, nu 10, lam0 1e-3, gtol 1e-8, ftol 1e-10, xtol 1e-10,
lam_max 1e16, max_iter 100) are those of the test problems; they are unmeasured on a real
retrieval.
"""
import types

import numpy as np

from ._capi import constant

MAX_PARAMS = constant('PB_RETRIEVAL_MAX_PARAMS')
MAX_TRIALS = constant('PB_LM_MAX_TRIALS')
CHUNK = constant('PB_LM_CHUNK')     # the lanes of cost_host, the staged points
RUNNING, GTOL, FTOL, XTOL, STALL, MAXIT = range(6)
STATUS_NAMES = ('RUNNING', 'GTOL', 'FTOL', 'XTOL', 'STALL', 'MAXIT')
DEFAULTS = dict(fd_step=1e-4, ntrial=4, nu=10.0, lam0=1e-3, gtol=1e-8, ftol=1e-10, xtol=1e-10,
                lam_min=1e-15, lam_max=1e16, max_iter=100)


def _settings(kw):
    bad = set(kw) - set(DEFAULTS)
    if bad:
        raise ValueError(f'unknown settings {sorted(bad)}: one of {sorted(DEFAULTS)}')
    s = types.SimpleNamespace(**{**DEFAULTS, **kw})
    s.ntrial, s.max_iter = int(s.ntrial), int(s.max_iter)
    if not 1 <= s.ntrial <= MAX_TRIALS:
        raise ValueError(f'{s.ntrial} trials: 1 to {MAX_TRIALS}')
    if not (s.nu > 1.0 and np.isfinite(s.nu)):
        raise ValueError('nu must be above 1')
    if not (s.fd_step > 0.0 and np.isfinite(s.fd_step)):
        raise ValueError('fd_step must be positive')
    if not s.lam0 > 0.0:
        raise ValueError('lam0 must be positive')
    return s


def check_problem(nfree, pmin, pmax, scale, fd_step):
    """-> (pmin, pmax, scale) as float64[nfree]; refused: nfree outside 1 .. 128, a scale that is
    not positive and finite, pmin > pmax, and a parameter with pmax_k - pmin_k < 2 h_k (neither
    difference would fit between the bounds)."""
    nfree = int(nfree)
    if not 1 <= nfree <= MAX_PARAMS:
        raise ValueError(f'{nfree} free parameters: 1 to {MAX_PARAMS}')
    pmin, pmax, scale = (np.broadcast_to(np.asarray(a, dtype=np.float64), (nfree,)).copy()
                         for a in (pmin, pmax, scale))
    if not np.all(np.isfinite(scale) & (scale > 0)):
        raise ValueError('scale must be positive and finite')
    with np.errstate(invalid='ignore'):
        narrow = ~(pmax - pmin >= 2.0 * fd_step * scale)
    if np.any(narrow):
        raise ValueError(f'parameters {list(np.where(narrow)[0])}: pmax - pmin < 2 h with '
                         f'h = fd_step scale = {list(fd_step * scale[narrow])}')
    return pmin, pmax, scale


# ------------------------------------------------------------------------------ one iteration
def probe_host(theta, pmax, scale, fd_step):
    """theta[ns, nfree] -> (probe[ns, nfree + 1, nfree], step[ns, nfree])."""
    theta = np.asarray(theta, dtype=np.float64)
    ns, nfree = theta.shape
    h = fd_step * np.asarray(scale, dtype=np.float64)
    step = np.where(theta + h > pmax, -h, h)
    probe = np.repeat(theta[:, None, :], nfree + 1, axis=1)
    k = np.arange(nfree)
    probe[:, k + 1, k] = theta + step
    return probe, step


def cost_host(R):
    """0.5 |R|^2 over the last axis in the kernels' order: 64 partial sums -- lane j takes
    i = j, j + 64, ... in index order --, then the butterfly v = v + v[lane ^ off] for
    off = 32, 16, .., 1."""
    R = np.asarray(R, dtype=np.float64)
    m = R.shape[-1]
    n = -(-m // CHUNK)
    sq = np.zeros(R.shape[:-1] + (n * CHUNK,))
    with np.errstate(all='ignore'):
        sq[..., :m] = R * R
        sq = sq.reshape(R.shape[:-1] + (n, CHUNK))
        v = np.zeros(R.shape[:-1] + (CHUNK,))
        for c in range(n):
            v = v + sq[..., c, :]
        lane = np.arange(CHUNK)
        off = CHUNK // 2
        while off:
            v = v + v[..., lane ^ off]
            off //= 2
        return 0.5 * v[..., 0]


def normal_host(R, step):
    """R[ns, nfree + 1, m], step[ns, nfree] -> (A[ns, nfree, nfree], g[ns, nfree], cost[ns])
    (module docstring: normal)."""
    R = np.asarray(R, dtype=np.float64)
    step = np.asarray(step, dtype=np.float64)
    ns, n1, m = R.shape
    nfree = n1 - 1
    with np.errstate(all='ignore'):
        D = R[:, 1:, :] - R[:, :1, :]                       # [ns, nfree, m]
        S = np.zeros((ns, nfree, nfree))
        gs = np.zeros((ns, nfree))
        for i in range(m):
            d = D[:, :, i]
            S = S + d[:, :, None] * d[:, None, :]
            gs = gs + d * R[:, 0, i, None]
        k = np.arange(nfree)
        lo, hi = np.minimum(k[:, None], k[None, :]), np.maximum(k[:, None], k[None, :])
        A = (S / step[:, lo]) / step[:, hi]
        g = gs / step
        frozen = ~np.all(np.isfinite(D), axis=2)
        A = np.where(frozen[:, :, None] | frozen[:, None, :], 0.0, A)
        g = np.where(frozen, 0.0, g)
    return A, g, cost_host(R[:, 0, :])


def normal_from_jacobian(J, R0):
    """The analytic form (lm_host's jac=, for tests only): J[ns, m, nfree], R0[ns, m] ->
    (A = J^T J, g = J^T R0, cost)."""
    J, R0 = np.asarray(J, dtype=np.float64), np.asarray(R0, dtype=np.float64)
    A = np.einsum('sik,sil->skl', J, J)
    A = 0.5 * (A + np.swapaxes(A, 1, 2))
    return A, np.einsum('sik,si->sk', J, R0), cost_host(R0)


def active_host(A, g, theta, pmin, pmax):
    """[.., nfree] bool: the parameters a step leaves alone."""
    diag = np.diagonal(A, axis1=-2, axis2=-1)
    return ((theta <= pmin) & (g > 0.0)) | ((theta >= pmax) & (g < 0.0)) | (diag == 0.0)


def cholesky_host(M, tol=0.0):
    """The lower factor of M[n, n] (its lower triangle is read), right-looking, or None at the
    first pivot that is not finite or not above tol M_pp (tol = 0: a pivot <= 0), M_pp the
    diagonal before the factorisation: column p is divided by sqrt(pivot), then
    M_ab -= M_ap M_bp for p < b <= a."""
    L = np.tril(np.array(M, dtype=np.float64))
    n = L.shape[0]
    d0 = np.diagonal(L).copy()
    with np.errstate(all='ignore'):
        for p in range(n):
            d = L[p, p]
            least = tol * d0[p] if tol > 0.0 else 0.0
            if not (d > least) or not np.isfinite(d):
                return None
            L[p, p] = np.sqrt(d)
            L[p + 1:, p] = L[p + 1:, p] / L[p, p]
            col = L[p + 1:, p]
            L[p + 1:, p + 1:] = np.tril(L[p + 1:, p + 1:] - col[:, None] * col[None, :])
    return L


def cholesky_solve_host(L, b):
    """x of L L^T x = b, column-oriented: y_p = b_p / L_pp, b_a -= L_ap y_p (a > p); then
    x_p = y_p / L_pp, y_a -= L_pa x_p (a < p), p descending."""
    x = np.array(b, dtype=np.float64)
    n = len(x)
    with np.errstate(all='ignore'):
        for p in range(n):
            x[p] = x[p] / L[p, p]
            x[p + 1:] = x[p + 1:] - L[p + 1:, p] * x[p]
        for p in range(n - 1, -1, -1):
            x[p] = x[p] / L[p, p]
            x[:p] = x[:p] - L[p, :p] * x[p]
    return x


def trial_lambda(lam, nu, j):
    """lam nu^(j-1) as the kernels form it: lam / nu, then times nu per trial."""
    lj = lam / nu
    for _ in range(int(j)):
        lj = lj * nu
    return lj


def step_host(A, g, theta, lam, pmin, pmax, scale, nu=10.0, ntrial=4):
    """-> (trial[ns, ntrial, nfree], pgrad[ns]) (module docstring: step)."""
    A, g, theta = (np.asarray(a, dtype=np.float64) for a in (A, g, theta))
    ns, nfree = theta.shape
    trial = np.repeat(theta[:, None, :], ntrial, axis=1)
    pgrad = np.zeros(ns)
    for s in range(ns):
        f = np.where(~active_host(A[s], g[s], theta[s], pmin, pmax))[0]
        if len(f) == 0:
            continue
        pgrad[s] = np.max(np.abs(g[s, f]) * scale[f])
        Af = A[s][np.ix_(f, f)]
        for j in range(ntrial):
            lj = trial_lambda(lam[s], nu, j)
            M = Af.copy()
            d = np.diagonal(Af)
            with np.errstate(all='ignore'):
                M[np.arange(len(f)), np.arange(len(f))] = d + lj * d
            L = cholesky_host(M)
            if L is None:
                continue
            delta = cholesky_solve_host(L, -g[s, f])
            if not np.all(np.isfinite(delta)):
                continue
            trial[s, j, f] = np.minimum(np.maximum(theta[s, f] + delta, pmin[f]), pmax[f])
    return trial, pgrad


def new_state_host(theta0, lam0=1e-3):
    theta = np.array(theta0, dtype=np.float64)
    ns = theta.shape[0]
    return types.SimpleNamespace(
        theta=theta, cost=np.full(ns, np.nan), lam=np.full(ns, float(lam0)),
        status=np.zeros(ns, np.int32), niter=np.zeros(ns, np.int32),
        picked=np.full(ns, -1, np.int32), unfinished=ns)


def update_host(st, trial, Rt, pgrad, scale, nu=10.0, lam_min=1e-15, lam_max=1e16, gtol=1e-8,
                ftol=1e-10, xtol=1e-10, max_iter=100):
    """The decision of every running start on the state st (theta, cost, lam, status, niter,
    picked, unfinished), in place; a finished start is left untouched (picked too).
        cost not finite: STALL; else pgrad <= gtol: GTOL -- both without a step (picked = -1,
        niter unchanged).
        Otherwise the trial costs (cost_host); the lowest finite one wins, ties to the lowest
        index.  Below cost: theta = that trial, cost = its cost, lam = max(lam_j / nu, lam_min);
        FTOL if cost_old - cost_new <= ftol max(cost_old, 1), else XTOL if
        max_k |dtheta_k| / scale_k <= xtol.  Else lam = lam nu^ntrial (one multiplication per
        trial).  niter += 1; still running and lam > lam_max: STALL; still running and
        niter >= max_iter: MAXIT."""
    trial, Rt = np.asarray(trial, dtype=np.float64), np.asarray(Rt, dtype=np.float64)
    ns, ntrial, _ = trial.shape
    tcost = cost_host(Rt)
    for s in range(ns):
        if st.status[s] != RUNNING:
            continue
        c0 = st.cost[s]
        if not np.isfinite(c0) or pgrad[s] <= gtol:
            st.status[s] = GTOL if np.isfinite(c0) else STALL
            st.picked[s] = -1
            continue
        best, cbest = -1, np.inf
        for j in range(ntrial):
            if np.isfinite(tcost[s, j]) and tcost[s, j] < cbest:
                best, cbest = j, tcost[s, j]
        status = RUNNING
        if best >= 0 and cbest < c0:
            dx = np.max(np.abs(trial[s, best] - st.theta[s]) / scale)
            st.theta[s] = trial[s, best]
            lam = max(trial_lambda(st.lam[s], nu, best) / nu, lam_min)
            if c0 - cbest <= ftol * max(c0, 1.0):
                status = FTOL
            elif dx <= xtol:
                status = XTOL
            st.cost[s] = cbest
        else:
            best = -1
            lam = st.lam[s]
            for _ in range(ntrial):
                lam = lam * nu
        st.niter[s] += 1
        if status == RUNNING and lam > lam_max:
            status = STALL
        if status == RUNNING and st.niter[s] >= max_iter:
            status = MAXIT
        st.lam[s], st.status[s], st.picked[s] = lam, status, best
    st.unfinished = int(np.sum(st.status == RUNNING))
    return st


def covariance_host(A, g, theta, pmin, pmax):
    """-> (C[ns, nfree, nfree], active[ns, nfree] int32, singular[ns] int32): C = (A_ff)^-1 on the
    parameters that are not active, 0 in the active rows and columns; Cholesky, one solve per
    column of the identity, the upper triangle mirrored.  Singular -- NaN in the free block and
    singular = 1 -- means numerically singular: a pivot that is not above nf eps A_pp (nf free
    parameters), which the rounding of the nf updates before it could have made; an
    underdetermined J^T J leaves pivots of either sign at that size."""
    A, g, theta = (np.asarray(a, dtype=np.float64) for a in (A, g, theta))
    ns, nfree = theta.shape
    C = np.zeros((ns, nfree, nfree))
    active = np.zeros((ns, nfree), np.int32)
    singular = np.zeros(ns, np.int32)
    for s in range(ns):
        act = active_host(A[s], g[s], theta[s], pmin, pmax)
        active[s] = act
        f = np.where(~act)[0]
        L = cholesky_host(A[s][np.ix_(f, f)], len(f) * np.finfo(float).eps)
        if L is None:
            singular[s] = 1
            C[s][np.ix_(f, f)] = np.nan
            continue
        X = np.zeros((len(f), len(f)))
        for c in range(len(f)):
            X[:, c] = cholesky_solve_host(L, np.eye(len(f))[c])
        X = np.triu(X) + np.triu(X, 1).T
        C[s][np.ix_(f, f)] = X
    return C, active, singular


def lm_host(residuals, theta0, pmin, pmax, scale, jac=None, niter=None, state=None, **kw):
    """The whole loop in NumPy.  residuals: theta[n, nfree] -> [n, m]; theta0[ns, nfree] (or
    [nfree]: one start); pmin, pmax, scale [nfree] (scalars broadcast); jac (tests only):
    theta[n, nfree] -> J[n, m, nfree], which replaces the probe points and the differences by
    normal_from_jacobian; kw: the settings of DEFAULTS.  It runs until every start has a status,
    or niter iterations if that is given; state= continues a run.  -> the state
    (new_state_host) with A, g, pgrad of the last iteration, .accepted (one picked[ns] per
    iteration) and .nresiduals, the residual calls so far."""
    s = _settings(kw)
    theta0 = np.atleast_2d(np.asarray(theta0, dtype=np.float64))
    nfree = theta0.shape[1]
    pmin, pmax, scale = check_problem(nfree, pmin, pmax, scale, s.fd_step)
    st = state
    if st is None:
        with np.errstate(invalid='ignore'):
            outside = ~np.all((theta0 >= pmin) & (theta0 <= pmax), axis=1)
        if np.any(outside):
            raise ValueError(f'starts {list(np.where(outside)[0])} are outside the bounds')
        st = new_state_host(theta0, s.lam0)
        st.accepted, st.nresiduals = [], 0
    done = 0
    while st.unfinished and (niter is None or done < int(niter)):
        if jac is None:
            probe, step = probe_host(st.theta, pmax, scale, s.fd_step)
            R = np.asarray(residuals(probe.reshape(-1, nfree)), dtype=np.float64)
            st.A, st.g, st.cost = normal_host(R.reshape(len(st.theta), nfree + 1, -1), step)
        else:
            R0 = np.asarray(residuals(st.theta), dtype=np.float64)
            st.A, st.g, st.cost = normal_from_jacobian(jac(st.theta), R0)
        trial, st.pgrad = step_host(st.A, st.g, st.theta, st.lam, pmin, pmax, scale, s.nu,
                                    s.ntrial)
        Rt = np.asarray(residuals(trial.reshape(-1, nfree)), dtype=np.float64)
        update_host(st, trial, Rt.reshape(len(st.theta), s.ntrial, -1), st.pgrad, scale, s.nu,
                    s.lam_min, s.lam_max, s.gtol, s.ftol, s.xtol, s.max_iter)
        st.accepted.append(st.picked.copy())
        st.nresiduals += 2
        done += 1
    return st


# ------------------------------------------------------------------------------ the device loop
class LevenbergMarquardt:
    """LevenbergMarquardt(residuals, nfree, pmin, pmax, scale, **settings): lm_host on the device.
    residuals: any callable from a float64 device tensor theta[n, nfree] to [n, m]
    (Retrieval.residuals, or torch arithmetic); scale: the parameters' natural step (Retrieval
    passes pstep of the free lines); settings: DEFAULTS (unmeasured on a real retrieval).

    start(theta0) takes the starts (one outside the bounds is refused).  run(niter): launches
    only, nothing read back; run(a) then run(b) leaves the bits of run(a + b).
    run_until(check_every, max_iter) reads back one int32, the number of unfinished starts, per
    check.  finish() -> (A, g, cost) at the final points; covariance() -> (C, active, singular).
    A finished start is still evaluated, so that the shapes stay fixed, and never changed."""

    def __init__(self, residuals, nfree, pmin, pmax, scale, **settings):
        self.residuals = residuals
        self.s = _settings(settings)
        self.nfree = int(nfree)
        self.pmin_host, self.pmax_host, self.scale_host = check_problem(
            nfree, pmin, pmax, scale, self.s.fd_step)
        self.ns = None
        self.trace = None           # a list: run() appends picked[ns] of every iteration

    def start(self, theta0):
        import torch
        from ._capi import call
        from ._device import dev, require_gpu
        require_gpu()
        theta0 = dev(theta0)
        if theta0.dim() != 2 or theta0.shape[1] != self.nfree or theta0.shape[0] < 1:
            raise ValueError(f'theta0 must have shape (ns >= 1, {self.nfree}), got '
                             f'{tuple(theta0.shape)}')
        self.pmin, self.pmax, self.scale = (dev(a) for a in (self.pmin_host, self.pmax_host,
                                                             self.scale_host))
        if not bool(((theta0 >= self.pmin) & (theta0 <= self.pmax)).all()):
            raise ValueError('theta0: a start is outside the bounds')
        ns, nfree, nt = theta0.shape[0], self.nfree, self.s.ntrial
        f64 = dict(dtype=torch.float64, device='cuda')
        i32 = dict(dtype=torch.int32, device='cuda')
        self.ns, self.m = ns, None
        self.theta = theta0.clone()
        self.cost = torch.full((ns,), float('nan'), **f64)
        self.lam = torch.full((ns,), float(self.s.lam0), **f64)
        self.status = torch.zeros(ns, **i32)
        self.niter = torch.zeros(ns, **i32)
        self.picked = torch.full((ns,), -1, **i32)
        self.unfinished = torch.full((1,), ns, **i32)
        self.probe = torch.empty((ns, nfree + 1, nfree), **f64)
        self.step = torch.empty((ns, nfree), **f64)
        self.A = torch.empty((ns, nfree, nfree), **f64)
        self.g = torch.empty((ns, nfree), **f64)
        self.pgrad = torch.empty(ns, **f64)
        self.trial = torch.empty((ns, nt, nfree), **f64)
        self.work = torch.empty(call('pb_lm_work_doubles', nfree, nt, ns), **f64)
        self.done = 0
        return self

    def _started(self):
        if self.ns is None:
            raise ValueError('LevenbergMarquardt: start() comes first')

    def _residuals(self, points, rows):
        import torch
        R = self.residuals(points.view(-1, self.nfree))
        if not isinstance(R, torch.Tensor) or not R.is_cuda or R.dtype != torch.float64 or \
                R.dim() != 2 or R.shape[0] != self.ns * rows or R.shape[1] < 1 or \
                (self.m is not None and R.shape[1] != self.m):
            raise ValueError(f'residuals must return a float64 device tensor of shape '
                             f'({self.ns * rows}, m >= 1), got {type(R).__name__} '
                             f'{getattr(R, "dtype", "")} {tuple(getattr(R, "shape", ()))}')
        self.m = R.shape[1]
        return R.contiguous()

    def _normal(self):
        from ._capi import call
        from ._device import _ptr, _stream
        call('pb_lm_probe', _ptr(self.probe), _ptr(self.step), _ptr(self.theta), _ptr(self.pmax),
             _ptr(self.scale), self.s.fd_step, self.nfree, self.ns, _stream())
        R = self._residuals(self.probe, self.nfree + 1)
        call('pb_lm_normal', _ptr(self.A), _ptr(self.g), _ptr(self.cost), _ptr(R),
             _ptr(self.step), self.nfree, self.m, self.ns, _stream())

    def run(self, niter):
        """niter more iterations: probe, residuals, normal, step, residuals, update; nothing read
        back."""
        from ._capi import call
        from ._device import _ptr, _stream
        self._started()
        s = self.s
        for _ in range(int(niter)):
            self._normal()
            call('pb_lm_step', _ptr(self.trial), _ptr(self.pgrad), _ptr(self.work), _ptr(self.A),
                 _ptr(self.g), _ptr(self.theta), _ptr(self.lam), _ptr(self.pmin),
                 _ptr(self.pmax), _ptr(self.scale), s.nu, s.ntrial, self.nfree, self.ns,
                 _stream())
            Rt = self._residuals(self.trial, s.ntrial)
            call('pb_lm_update', _ptr(self.theta), _ptr(self.cost), _ptr(self.lam),
                 _ptr(self.status), _ptr(self.niter), _ptr(self.picked), _ptr(self.unfinished),
                 _ptr(self.trial), _ptr(Rt), _ptr(self.pgrad), _ptr(self.scale), s.nu, s.lam_min,
                 s.lam_max, s.gtol, s.ftol, s.xtol, s.max_iter, s.ntrial, self.nfree, self.m,
                 self.ns, _stream())
            if self.trace is not None:
                self.trace.append(self.picked.clone())
            self.done += 1
        return self

    def run_until(self, check_every=5, max_iter=None):
        """Iterations until no start is running, looked at after every check_every-th iteration
        (one int32 read back per look); max_iter (default: the setting) at the most, after which
        every start has a status."""
        self._started()
        check_every = int(check_every)
        if check_every < 1:
            raise ValueError('check_every >= 1')
        if max_iter is not None:
            self.s.max_iter = int(max_iter)
        cap = self.s.max_iter
        done = 0
        while done < cap:
            step = min(check_every, cap - done)
            self.run(step)
            done += step
            if self.unfinished.item() == 0:
                break
        return self

    def finish(self):
        """(A, g, cost) at the current points: one probe, residual and normal call."""
        self._started()
        self._normal()
        return self.A, self.g, self.cost

    def covariance(self):
        """(C[ns, nfree, nfree], active[ns, nfree] int32, singular[ns] int32) at the current
        points (covariance_host), after finish()."""
        import torch
        from ._capi import call
        from ._device import _ptr, _stream
        self.finish()
        ns, nfree = self.ns, self.nfree
        C = torch.empty((ns, nfree, nfree), dtype=torch.float64, device='cuda')
        active = torch.empty((ns, nfree), dtype=torch.int32, device='cuda')
        singular = torch.empty(ns, dtype=torch.int32, device='cuda')
        call('pb_lm_covariance', _ptr(C), _ptr(active), _ptr(singular), _ptr(self.work),
             _ptr(self.A), _ptr(self.g), _ptr(self.theta), _ptr(self.pmin), _ptr(self.pmax),
             nfree, ns, _stream())
        return C, active, singular


class Optimum:
    """What Retrieval.optimize returns: the device tensors theta[ns, nfree], cost[ns],
    log_posterior[ns], status[ns] (STATUS_NAMES), niter[ns], covariance[ns, nfree, nfree],
    active[ns, nfree], singular[ns]; best(), the index of the largest finite log-posterior (found
    on the device, one read-back); bestp(), the full parameter vector of that start (the
    reference's `bestp`)."""

    def __init__(self, retrieval, lm, log_posterior, covariance, active, singular):
        self.retrieval, self.lm = retrieval, lm
        self.theta, self.cost, self.status, self.niter = lm.theta, lm.cost, lm.status, lm.niter
        self.log_posterior = log_posterior
        self.covariance, self.active, self.singular = covariance, active, singular
        self._best = None

    def best(self):
        import torch
        if self._best is None:
            lp = self.log_posterior
            key = torch.where(torch.isfinite(lp), lp, torch.full_like(lp, -float('inf')))
            top, i = torch.max(key, dim=0)
            top, i = torch.stack((top, i.to(torch.float64))).cpu().numpy()
            if not np.isfinite(top):
                raise ValueError('Optimum: no start has a finite log-posterior')
            self._best = int(i)
        return self._best

    def bestp(self):
        theta = self.theta[self.best()].cpu().numpy()
        return self.retrieval.expand_host(theta[None, :])[0]
