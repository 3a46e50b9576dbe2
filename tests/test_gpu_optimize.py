"""The optimiser on the device (csrc/pb_optimize.hip, pyratbay_amd/optimize.py) against its NumPy
statements, at the C ABI on NaN-filled outputs with a guard row behind them:

  * pb_lm_residuals against retrieval.residual_rows_host;
  * pb_lm_probe and pb_lm_normal against probe_host / normal_host: symmetric in bits, two runs in
    bits, the error in units of eps sum |J_ik J_il|;
  * pb_lm_step against step_host and the 50-digit solves of optimize_cases (units of cond eps);
  * pb_lm_update against update_host over 50 successive calls, exactly;
  * pb_lm_covariance against covariance_host and C A - 1;
  * LevenbergMarquardt on torch callables of the CPU problems against lm_host;
  * Retrieval.optimize on the small emission retrieval.

Measured on the device (profiles/optimize.md).  The kernels round every product and sum on its
own, in the order of the statements, and division and square root are correctly rounded: A, g,
cost, the trial points and the covariance came out with the HOST'S BITS in every case here, so
the measured worst error against the host statement is 0 units and, by the project's rule (the
next power of two above four times the measured worst), so is the committed bound: equality.
Against the 50-digit solves the device then has the host's error, 1.667 units of cond eps at
the worst (test_optimize_cpu), and 1.752 units for the residual of the damped system: the bound
is 8 units for both; C A - 1 in the diagonal scaling is within 0.25 units of n cond eps: 1 unit."""
import numpy as np
import pytest

import optimize_cases as oc

pytestmark = pytest.mark.gpu

EPS = oc.EPS
NORMAL_UNITS = 0.0          # against the host statement: the host's bits (module docstring)
SOLVE_UNITS = 8.0           # against 50 digits, units of cond eps: measured 1.667
SOLVE_RESIDUAL_UNITS = 8.0  # |(A + lam D) delta + g| scaled, units of cond eps: measured 1.752
COV_UNITS = 1.0             # |W C A W^-1 - 1|, units of n cond eps: measured 0.24999999999999994


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def _torch():
    import torch
    return torch


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """Equal as bit patterns, with any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def nan_tensor(shape):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')


def int_tensor(shape, value=-77):
    import torch
    return torch.full(shape, value, dtype=torch.int32, device='cuda')


_ALIVE = []


def U(eng, a):
    """The device pointer of an uploaded host array; the tensor lives until the call has ended
    (a temporary would hand its memory to the next upload)."""
    _ALIVE.append(eng.dev(a))
    return P(_ALIVE[-1])


def call(name, *args):
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _stream
    import torch
    _capi.call(name, *args, _stream())
    torch.cuda.synchronize()
    _ALIVE.clear()


def P(t):
    from pyratbay_amd._device import _ptr
    return _ptr(t)


# -------------------------------------------------------------------------------------------------
# pb_lm_residuals
# -------------------------------------------------------------------------------------------------
def residual_case(ndata, ngauss, nw, nfree=4):
    from pyratbay_amd import observation as po
    rng = np.random.default_rng(100 * ndata + 10 * ngauss + nw)
    inst = ['nrs1', 'nrs2', 'miri']
    names = [f'{inst[b % 3]} {b}' for b in range(ndata)]
    offs = ['offset_nrs1'] + (['offset_miri'] if ndata >= 3 else [])
    errs = ['err_scale_nrs1'] if ndata < 3 else ['err_scale_nrs2', 'err_quad_miri']
    obs = po.Observation(rng.uniform(1.0, 2.0, ndata), rng.uniform(0.1, 0.5, ndata), names, offs,
                         errs, units='percent')
    theta = rng.normal(0, 1, (nw, nfree))
    model = obs.data_host + rng.normal(0, 1, (nw, ndata))
    offsets = rng.uniform(-20, 20, (nw, obs.noff))
    err_pars = rng.uniform(-0.5, 1.5, (nw, obs.nerr))
    gauss = np.arange(nfree)[::-1][:ngauss].astype(np.int32).copy()
    prior, lo, up = rng.normal(0, 1, nfree), rng.uniform(0.1, 2, nfree), rng.uniform(0.1, 2, nfree)
    return obs, theta, model, offsets, err_pars, gauss, prior, lo, up


def run_residuals(eng, obs, theta, inside, model, offsets, err_pars, gauss, prior, lo, up):
    nw, nfree = theta.shape
    m = obs.nbands + len(gauss)
    out = nan_tensor((nw + 1, m))
    d = obs._resident()
    t = [eng.dev(a) for a in (model, offsets, err_pars, theta, prior, lo, up)]
    ins, gi = eng.dev(inside, _torch().int32), eng.dev(gauss, _torch().int32)
    call('pb_lm_residuals', P(out), P(t[0]), P(d['data']), P(d['uncert']), P(d['offset_group']),
         P(t[1]), obs.unit, obs.noff, P(d['err_group']), P(d['err_mode']), P(t[2]), obs.unit,
         obs.nerr, P(t[3]), P(ins), P(gi) if len(gauss) else None, P(t[4]), P(t[5]), P(t[6]),
         len(gauss), nfree, nw, obs.nbands)
    assert bool(_torch().isnan(out[nw]).all())
    return host(out[:nw])


@pytest.mark.parametrize('nw', [1, 5])
@pytest.mark.parametrize('ngauss', [0, 1, 4])
@pytest.mark.parametrize('ndata', [1, 3, 65])
def test_residuals_against_the_host_statement(eng, ndata, ngauss, nw):
    """|dR| <= eps (2 (|d| + |o unit| + |m|) / u + 8 |R|): the roundings of the numerator, and of
    the quotient and the scaled uncertainty (pow within 2 ulp, a product, a square root)."""
    from pyratbay_amd import retrieval as pr
    obs, theta, model, offsets, err_pars, gauss, prior, lo, up = residual_case(ndata, ngauss, nw)
    inside = np.ones(nw, np.int32)
    want = pr.residual_rows_host(obs, theta, inside, model, offsets, err_pars, gauss, prior, lo, up)
    got = run_residuals(eng, obs, theta, inside, model, offsets, err_pars, gauss, prior, lo, up)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    nd = obs.nbands
    assert np.array_equal(bits(got[:, nd:]), bits(want[:, nd:]))            # the prior columns
    worst = 0.0
    for w in range(nw):
        u = obs.scale_errors_host(err_pars[w])
        mag = np.abs(obs.data_host) + np.abs(obs.offset_data_host(offsets[w]) - obs.data_host) + \
            np.abs(model[w])
        bound = EPS * (2.0 * mag / u + 8.0 * np.abs(want[w, :nd]))
        worst = max(worst, float(np.max(np.abs(got[w, :nd] - want[w, :nd]) / bound)))
    print(f'residuals ndata {ndata} ngauss {ngauss} nw {nw}: worst {worst:.3f} of the bound')
    assert worst <= 1.0
    # a rejected model and a walker outside: rows of +inf, nothing behind the guard
    if nw > 1:
        model[1, ndata // 2] = np.inf
        inside[nw - 1] = 0
        want = pr.residual_rows_host(obs, theta, inside, model, offsets, err_pars, gauss, prior,
                                     lo, up)
        got2 = run_residuals(eng, obs, theta, inside, model, offsets, err_pars, gauss, prior, lo,
                             up)
        assert np.all(got2[1] == np.inf) and np.all(got2[nw - 1] == np.inf)
        assert np.array_equal(np.isinf(got2), np.isinf(want))
        assert np.array_equal(bits(got2[0]), bits(got[0]))


def test_residuals_refusals(eng):
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _stream
    t = eng.dev(np.zeros(8))
    a = [P(t)] * 6
    with pytest.raises(_capi.PbError, match='129 free parameters: 1 to 128'):
        _capi.call('pb_lm_residuals', *a, 1.0, 0, None, None, None, 1.0, 0, *a, 0, 129, 1, 1,
                   _stream())
    with pytest.raises(_capi.PbError, match='null pointer'):
        _capi.call('pb_lm_residuals', None, *a[1:], 1.0, 0, None, None, None, 1.0, 0, *a, 0, 2, 1,
                   1, _stream())
    with pytest.raises(_capi.PbError, match=r'null pointer \(priors\)'):
        _capi.call('pb_lm_residuals', *a, 1.0, 0, None, None, None, 1.0, 0, *a[:2], None, *a[:3],
                   1, 2, 1, 1, _stream())
    _capi.call('pb_lm_residuals', *([None] * 6), 1.0, 0, None, None, None, 1.0, 0, *([None] * 6),
               0, 2, 0, 1, _stream())


# -------------------------------------------------------------------------------------------------
# pb_lm_probe, pb_lm_normal
# -------------------------------------------------------------------------------------------------
def run_normal(eng, R, step):
    ns, n1, m = R.shape
    nfree = n1 - 1
    A, g, cost = nan_tensor((ns + 1, nfree, nfree)), nan_tensor((ns + 1, nfree)), \
        nan_tensor((ns + 1,))
    call('pb_lm_normal', P(A), P(g), P(cost), U(eng, R), U(eng, step), nfree, m, ns)
    torch = _torch()
    assert bool(torch.isnan(A[ns]).all()) and bool(torch.isnan(g[ns]).all())
    assert bool(torch.isnan(cost[ns]))
    return host(A[:ns]), host(g[:ns]), host(cost[:ns])


NORMAL_WORST = {'A': 0.0, 'g': 0.0, 'cost': 0.0}


@pytest.mark.parametrize('nfree', oc.NORMAL_NFREES)
def test_normal_against_the_host_statement(eng, nfree):
    """m straddles PB_LM_CHUNK = 64 (63, 64, 65), the wavefront, a block of 256 and many chunks
    (4099 = 64 * 64 + 3); nfree the 2 x 2 thread tile and the 32 x 32 block tile."""
    from pyratbay_amd import optimize as po
    assert po.CHUNK == 64
    for m in oc.NORMAL_MS:
        for ns in oc.NORMAL_NS:
            R, step = oc.normal_case(nfree, m, ns, 1000 * nfree + 10 * m + ns)
            assert np.any(step < 0) and np.ptp(np.log10(np.abs(step))) > (2 if nfree > 2 else -1)
            want_A, want_g, want_cost = po.normal_host(R, step)
            A, g, cost = run_normal(eng, R, step)
            assert np.all(np.isfinite(A)) and np.all(np.isfinite(g))
            assert np.array_equal(bits(A), bits(np.swapaxes(A, 1, 2)))      # symmetric in bits
            A2, g2, cost2 = run_normal(eng, R, step)
            assert same_bits(A, A2) and same_bits(g, g2) and same_bits(cost, cost2)
            # the frozen column of the last start
            assert np.all(A[ns - 1, nfree - 1] == 0) and np.all(A[ns - 1, :, nfree - 1] == 0)
            assert g[ns - 1, nfree - 1] == 0 and np.all(np.isfinite(cost))
            assert np.all(np.diagonal(A, axis1=1, axis2=2)[:ns - 1] > 0)
            with np.errstate(all='ignore'):
                J = (R[:, 1:] - R[:, :1]) / step[:, :, None]
                J = np.where(np.isfinite(J), J, 0.0)
                r0 = np.where(np.isfinite(R[:, 0]), R[:, 0], 0.0)
                sa = np.einsum('ski,sli->skl', np.abs(J), np.abs(J))
                sg = np.einsum('ski,si->sk', np.abs(J), np.abs(r0))
                sc = 0.5 * np.sum(r0 * r0, axis=1)
            live = np.isfinite(want_cost)
            ua = np.max(np.abs(A - want_A) / (EPS * np.where(sa > 0, sa, 1.0)))
            ug = np.max(np.abs(g - want_g) / (EPS * np.where(sg > 0, sg, 1.0)))
            uc = np.max(np.abs(cost - want_cost)[live] / (EPS * sc[live]), initial=0.0)
            for key, u in (('A', ua), ('g', ug), ('cost', uc)):
                NORMAL_WORST[key] = max(NORMAL_WORST[key], float(u))
            assert ua <= NORMAL_UNITS and ug <= NORMAL_UNITS and uc <= NORMAL_UNITS
            assert same_bits(cost, want_cost)
    print(f'normal nfree {nfree}: largest errors so far {NORMAL_WORST} units')


def test_normal_of_a_start_without_a_finite_residual(eng):
    from pyratbay_amd import optimize as po
    R, step = oc.normal_case(5, 70, 3, 4)
    R[1, :, :] = np.inf                                       # outside, or a rejected model
    R[0, 0, 69] = np.nan
    want = po.normal_host(R, step)
    got = run_normal(eng, R, step)
    for a, b in zip(got, want):
        assert same_bits(a, b)
    A, g, cost = got
    assert np.all(A[:2] == 0) and np.all(g[:2] == 0) and cost[1] == np.inf and np.isnan(cost[0])
    assert np.all(A[2, :4, :4] != 0) and np.all(A[2, 4] == 0)


def test_probe_and_refusals(eng):
    from pyratbay_amd import _capi, optimize as po
    from pyratbay_amd._device import _stream
    rng = np.random.default_rng(8)
    for nfree, ns in ((1, 1), (3, 5), (128, 2)):
        scale = 10.0**rng.uniform(-2, 2, nfree)
        pmax = np.full(nfree, 1.0)
        theta = rng.uniform(-1, 1, (ns, nfree))
        theta[0, 0] = 1.0 - 0.5e-4 * scale[0]                # theta + h > pmax: backward
        theta[ns - 1, nfree - 1] = 1.0
        want, want_step = po.probe_host(theta, pmax, scale, 1e-4)
        assert want_step[0, 0] < 0 and want_step[ns - 1, nfree - 1] < 0
        probe, step = nan_tensor((ns + 1, nfree + 1, nfree)), nan_tensor((ns + 1, nfree))
        call('pb_lm_probe', P(probe), P(step), U(eng, theta), U(eng, pmax),
             U(eng, scale), 1e-4, nfree, ns)
        assert np.all(np.isnan(host(probe[ns]))) and np.all(np.isnan(host(step[ns])))
        assert same_bits(host(probe[:ns]), want) and same_bits(host(step[:ns]), want_step)
    t = eng.dev(np.zeros(4))
    a = [P(t)] * 5
    with pytest.raises(_capi.PbError, match='m >= 1'):
        _capi.call('pb_lm_normal', *a, 2, 0, 1, _stream())
    with pytest.raises(_capi.PbError, match='0 free parameters: 1 to 128'):
        _capi.call('pb_lm_normal', *a, 0, 1, 1, _stream())
    with pytest.raises(_capi.PbError, match='null pointer'):
        _capi.call('pb_lm_normal', None, *a[1:], 1, 1, 1, _stream())
    with pytest.raises(_capi.PbError, match='fd_step must be positive'):
        _capi.call('pb_lm_probe', *a, 0.0, 1, 1, _stream())
    with pytest.raises(_capi.PbError, match='17 trials: 1 to 16'):
        _capi.call('pb_lm_step', *([P(t)] * 10), 10.0, 17, 1, 1, _stream())
    with pytest.raises(_capi.PbError, match='nu must be above 1'):
        _capi.call('pb_lm_step', *([P(t)] * 10), 1.0, 4, 1, 1, _stream())
    _capi.call('pb_lm_normal', *([None] * 5), 2, 3, 0, _stream())
    assert _capi.call('pb_lm_work_doubles', 128, 4, 3) == 3 * 4 * 128 * 128
    assert _capi.call('pb_lm_work_doubles', 5, 1, 2) == 2 * 2 * 25


# -------------------------------------------------------------------------------------------------
# pb_lm_step
# -------------------------------------------------------------------------------------------------
def run_step(eng, A, g, theta, lam, pmin, pmax, scale, nu, ntrial):
    from pyratbay_amd import _capi
    ns, nfree = theta.shape
    trial, pgrad = nan_tensor((ns + 1, ntrial, nfree)), nan_tensor((ns + 1,))
    work = nan_tensor((_capi.call('pb_lm_work_doubles', nfree, ntrial, ns),))
    call('pb_lm_step', P(trial), P(pgrad), P(work), U(eng, A), U(eng, g),
         U(eng, theta), U(eng, lam), U(eng, pmin), U(eng, pmax),
         U(eng, scale), nu, ntrial, nfree, ns)
    assert np.all(np.isnan(host(trial[ns]))) and np.isnan(host(pgrad[ns]))
    return host(trial[:ns]), host(pgrad[:ns])


@pytest.mark.parametrize('nfree', oc.SOLVE_NFREES)
def test_step_against_the_host_and_50_digits(eng, nfree):
    from pyratbay_amd import optimize as po
    cases = [oc.solve_case(nfree, cond) for cond in oc.SOLVE_CONDS]
    A, g, theta = (np.stack([getattr(c, k) for c in cases]) for k in ('A', 'g', 'theta'))
    c0 = cases[0]
    lam = np.full(3, oc.SOLVE_LAM)
    want, want_pg = po.step_host(A, g, theta, lam, c0.pmin, c0.pmax, c0.scale, oc.SOLVE_NU,
                                 oc.SOLVE_NTRIAL)
    got, pg = run_step(eng, A, g, theta, lam, c0.pmin, c0.pmax, c0.scale, oc.SOLVE_NU,
                       oc.SOLVE_NTRIAL)
    assert np.all(np.isfinite(got))                       # (a zero column: no NaN anywhere)
    assert same_bits(pg, want_pg)
    worst = dict(exact=0.0, residual=0.0, host=0.0)
    measured = 0
    for s, c in enumerate(cases):
        active = po.active_host(c.A, c.g, c.theta, c.pmin, c.pmax)
        assert np.array_equal(bits(got[s][:, active]), bits(np.tile(c.theta[active], (4, 1))))
        assert np.all(got[s] >= c.pmin) and np.all(got[s] <= c.pmax)
        assert np.all(c.theta == 0.0)             # a trial point is the step itself, unrounded
        for j in range(oc.SOLVE_NTRIAL):
            f, exact, kappa = oc.solve_exact(nfree, c.cond, j)
            clipped = (exact > c.pmax[f]) | (exact < c.pmin[f])
            # clipping is exact
            bound = np.where(exact > c.pmax[f], c.pmax[f], c.pmin[f])
            assert np.array_equal(got[s, j, f][clipped], bound[clipped])
            assert np.array_equal(got[s, j, f][clipped], want[s, j, f][clipped])
            ok = ~clipped
            delta, delta_host = got[s, j, f], want[s, j, f]
            w = np.sqrt(np.diag(c.A)[f])
            norm = np.linalg.norm((w * exact)[ok])
            u_exact = np.linalg.norm((w * (delta - exact))[ok]) / norm / (kappa * EPS)
            u_host = np.linalg.norm((w * (delta - delta_host))[ok]) / norm / (kappa * EPS)
            worst['exact'] = max(worst['exact'], u_exact)
            worst['host'] = max(worst['host'], u_host)
            assert u_exact <= SOLVE_UNITS
            assert u_host == 0.0
            if not clipped.any():
                lj = oc.trial_lam(j)
                Af = c.A[np.ix_(f, f)]
                M = Af.copy()
                np.fill_diagonal(M, np.diag(Af) * (1 + lj))
                r = (M @ delta + c.g[f]) / w
                u_res = np.linalg.norm(r) / np.linalg.norm(c.g[f] / w) / (kappa * EPS)
                worst['residual'] = max(worst['residual'], u_res)
                assert u_res <= SOLVE_RESIDUAL_UNITS
                measured += 1
    assert measured >= 4
    assert same_bits(got, want)
    print(f'step nfree {nfree}: worst units of cond eps {worst}')


def test_step_failed_pivot_and_clipping(eng):
    from pyratbay_amd import optimize as po
    A = np.array([[[1.0, 2.0], [2.0, 1.0]], [[4.0, 1.0], [1.0, 3.0]], [[0.0, 0.0], [0.0, 0.0]]])
    g = np.array([[0.3, -0.2], [8.0, -9.0], [0.0, 0.0]])
    theta = np.array([[0.1, 0.2], [-0.5, 0.5], [0.3, 0.3]])
    lo, hi, scale = np.full(2, -1.0), np.full(2, 1.0), np.ones(2)
    lam = np.full(3, 1e-3)
    want, want_pg = po.step_host(A, g, theta, lam, lo, hi, scale)
    got, pg = run_step(eng, A, g, theta, lam, lo, hi, scale, 10.0, 4)
    assert np.array_equal(bits(got[0]), bits(np.tile(theta[0], (4, 1))))   # indefinite: theta
    assert np.any(np.abs(got[1]) == 1.0)                                    # clipped
    assert np.array_equal(bits(got[2]), bits(np.tile(theta[2], (4, 1))))   # nothing free
    assert same_bits(got, want) and same_bits(pg, want_pg) and pg[2] == 0.0


# -------------------------------------------------------------------------------------------------
# pb_lm_update
# -------------------------------------------------------------------------------------------------
def test_update_over_50_calls(eng):
    from pyratbay_amd import optimize as po
    torch = _torch()
    ns, nfree, ntrial, m = 12, 3, 4, 70
    rng = np.random.default_rng(12)
    kw = dict(nu=10.0, lam_min=1e-15, lam_max=1e16, gtol=1e-8, ftol=1e-10, xtol=1e-10,
              max_iter=30)
    scale = np.array([0.1, 1.0, 10.0])
    st = po.new_state_host(rng.normal(0, 1, (ns, nfree)), 1e-3)
    rcur = rng.normal(0, 1, (ns, m))
    rcur[4, 7] = np.inf                                       # a start at an infinite cost
    st.cost = po.cost_host(rcur)
    d = dict(theta=eng.dev(np.vstack((st.theta, np.full((1, nfree), np.nan)))),
             cost=eng.dev(np.append(st.cost, np.nan)), lam=eng.dev(np.append(st.lam, np.nan)),
             status=eng.dev(np.append(st.status, -77), torch.int32),
             niter=eng.dev(np.append(st.niter, -77), torch.int32),
             picked=int_tensor((ns + 1,)), unfinished=int_tensor((2,)))
    seen = set()
    for it in range(50):
        factor = rng.uniform(0.8, 1.25, (ns, ntrial))
        factor[5, 1] = factor[5, 2] = 0.7                     # a tie of the two lowest costs
        Rt = rcur[:, None, :] * factor[:, :, None]
        Rt[3] = np.inf                                        # never a finite trial: stalls
        if it % 7 == 6:
            Rt[6] = np.nan
        trial = st.theta[:, None, :] + rng.normal(0, 0.3, (ns, ntrial, nfree)) * scale
        pgrad = rng.uniform(0.1, 1.0, ns)
        if it == 3:
            pgrad[0] = 1e-9                                   # GTOL
        if it == 5:
            Rt[1] = rcur[1] * (1.0 - 1e-13)                   # a tiny decrease: FTOL
        if it == 7:
            Rt[2, 0] = rcur[2] * 0.5                          # a tiny step: XTOL
            Rt[2, 1:] = rcur[2] * 0.9
            trial[2] = st.theta[2] + 1e-12 * scale
        before = (st.theta.copy(), st.cost.copy(), st.lam.copy(), st.status.copy())
        po.update_host(st, trial, Rt, pgrad, scale, **kw)
        for s in range(ns):
            if st.picked[s] >= 0 and before[3][s] == po.RUNNING:
                rcur[s] = Rt[s, st.picked[s]]
        call('pb_lm_update', P(d['theta']), P(d['cost']), P(d['lam']), P(d['status']),
             P(d['niter']), P(d['picked']), P(d['unfinished']), U(eng, trial),
             U(eng, Rt), U(eng, pgrad), U(eng, scale), kw['nu'], kw['lam_min'],
             kw['lam_max'], kw['gtol'], kw['ftol'], kw['xtol'], kw['max_iter'], ntrial, nfree, m,
             ns)
        assert same_bits(host(d['theta'][:ns]), st.theta), it
        assert same_bits(host(d['cost'][:ns]), st.cost), it
        assert same_bits(host(d['lam'][:ns]), st.lam), it
        assert np.array_equal(host(d['status'][:ns]), st.status), it
        assert np.array_equal(host(d['niter'][:ns]), st.niter), it
        running = before[3] == po.RUNNING
        assert np.array_equal(host(d['picked'][:ns])[running], st.picked[running]), it
        assert list(host(d['unfinished'])) == [st.unfinished, -77]
        # the guard row
        assert np.all(np.isnan(host(d['theta'][ns]))) and np.isnan(host(d['cost'][ns]))
        assert int(d['status'][ns]) == -77 and int(d['niter'][ns]) == -77
        assert int(d['picked'][ns]) == -77
        # a finished start is never changed again
        done = ~running
        assert same_bits(st.theta[done], before[0][done]) and same_bits(st.cost[done],
                                                                         before[1][done])
        seen |= set(st.status)
        if it == 4:
            assert st.picked[5] == 1                          # the lowest index wins the tie
    assert st.status[0] == po.GTOL and st.status[1] == po.FTOL and st.status[2] == po.XTOL
    assert st.status[3] == po.STALL and st.status[4] == po.STALL and st.niter[4] == 0
    assert seen == {po.RUNNING, po.GTOL, po.FTOL, po.XTOL, po.STALL, po.MAXIT}
    assert st.unfinished == 0 and np.max(st.niter) == 30


# -------------------------------------------------------------------------------------------------
# pb_lm_covariance
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nfree', oc.SOLVE_NFREES)
def test_covariance(eng, nfree):
    from pyratbay_amd import _capi, optimize as po
    torch = _torch()
    cases = [oc.solve_case(nfree, cond) for cond in oc.SOLVE_CONDS]
    A, g, theta = (np.stack([getattr(c, k) for c in cases] + [getattr(cases[0], k)])
                   for k in ('A', 'g', 'theta'))
    A[3] = -A[3]                                              # not positive definite: singular
    ns = 4
    c0 = cases[0]
    want, want_active, want_singular = po.covariance_host(A, g, theta, c0.pmin, c0.pmax)
    C = nan_tensor((ns + 1, nfree, nfree))
    active, singular = int_tensor((ns + 1, nfree)), int_tensor((ns + 1,))
    work = nan_tensor((_capi.call('pb_lm_work_doubles', nfree, 1, ns),))
    call('pb_lm_covariance', P(C), P(active), P(singular), P(work), U(eng, A), U(eng, g),
         U(eng, theta), U(eng, c0.pmin), U(eng, c0.pmax), nfree, ns)
    assert bool(torch.isnan(C[ns]).all()) and bool((active[ns] == -77).all())
    assert int(singular[ns]) == -77
    C, active, singular = host(C[:ns]), host(active[:ns]), host(singular[:ns])
    assert np.array_equal(active, want_active) and np.array_equal(singular, want_singular)
    assert list(singular) == [0, 0, 0, 1]
    worst = 0.0
    for s in range(ns):
        act = active[s] == 1
        f = np.where(~act)[0]
        assert np.all(C[s][act] == 0) and np.all(C[s][:, act] == 0)
        if singular[s]:
            assert np.all(np.isnan(C[s][np.ix_(f, f)]))
            continue
        assert np.all(np.isfinite(C[s])) and np.array_equal(bits(C[s]), bits(C[s].T))
        Af = A[s][np.ix_(f, f)]
        w = np.sqrt(np.diag(Af))
        kappa = np.linalg.cond(Af / w[:, None] / w[None, :])
        resid = (C[s][np.ix_(f, f)] @ Af - np.eye(len(f))) * w[:, None] / w[None, :]
        units = float(np.max(np.abs(resid))) / (len(f) * kappa * EPS)
        worst = max(worst, units)
        assert units <= COV_UNITS
    assert same_bits(C, want)
    print(f'covariance nfree {nfree}: worst {worst:.3f} units of n cond eps')


# -------------------------------------------------------------------------------------------------
# the loop
# -------------------------------------------------------------------------------------------------
LOOP_STARTS = {
    'rosenbrock': np.vstack((oc.ROSENBROCK_STARTS, [[1.5, 1.5]])),
    'bounded': np.vstack((oc.ROSENBROCK_STARTS, [[0.2, 2.0]])) * [1.0, 1.0],
    'expfit': np.vstack((oc.FIT_STARTS, [[2.0, -2.0, 0.2], [1.2, -0.5, 0.8]])),
}
LOOP_STARTS['bounded'][:, 0] = np.minimum(LOOP_STARTS['bounded'][:, 0], 0.5)
# The classes of a final status.  GTOL, FTOL, XTOL and STALL all say that the loop stopped AT a
# point by a criterion of its own; MAXIT says it ran out of iterations, RUNNING that it has not
# ended.  Which of the four fires at a minimum is decided by trial costs that tie to rounding
# there (torch.exp and numpy.exp differ by an ulp): with no trial strictly below the cost every
# iteration is a reject, lam grows by nu^ntrial per iteration and the start ends with STALL at the
# very cost lm_host ended at with FTOL (measured: the exponential fit's first start, 10 iterations
# on the device, 6 on the host).  So the four are one class, and the cost and parameter bounds
# below say that the point is the host's.
AT_A_POINT = {1, 2, 3, 4}


def status_class(status):
    return ['at a point' if s in AT_A_POINT else int(s) for s in status]


@pytest.mark.parametrize('name', list(LOOP_STARTS))
def test_loop_against_lm_host(eng, name):
    from pyratbay_amd import optimize as po
    res, jac, pmin, pmax, scale, _ = oc.PROBLEMS[name]
    starts = LOOP_STARTS[name]
    assert len(starts) == 5
    want = po.lm_host(res, starts, pmin, pmax, scale)
    lm = eng.LevenbergMarquardt(res, starts.shape[1], pmin, pmax, scale).start(starts)
    lm.run_until(check_every=7)
    status, cost, theta = host(lm.status), host(lm.cost), host(lm.theta)
    print(f'{name}: device iterations {list(host(lm.niter))} status {list(status)}; host '
          f'{list(want.niter)} {list(want.status)}')
    assert status_class(status) == status_class(want.status)
    assert all(c == 'at a point' for c in status_class(status))
    assert np.all(np.isfinite(cost)) and np.all(np.isfinite(want.cost))
    assert int(lm.unfinished.item()) == 0
    for s in range(5):
        gap = oc.gap_bounds(cost[s], want.cost[s])
        assert abs(cost[s] - want.cost[s]) <= gap, (s, cost[s], want.cost[s])
        J = jac(want.theta[s:s + 1])[0]
        A = J.T @ J
        if name == 'bounded' and want.theta[s, 0] == 0.5:
            assert theta[s, 0] == 0.5
            A[0, :] = A[:, 0] = 0.0
        D = theta[s] - want.theta[s]
        assert 0.5 * D @ A @ D <= oc.PARAMETER_GAP_FACTOR * gap, (s, D)
    assert np.all(theta >= np.broadcast_to(pmin, theta.shape))
    assert np.all(theta <= np.broadcast_to(pmax, theta.shape))


def test_loop_in_two_parts_and_the_read_back(eng, monkeypatch):
    torch = _torch()
    res, jac, pmin, pmax, scale, _ = oc.PROBLEMS['expfit']
    starts = LOOP_STARTS['expfit']

    def make():
        return eng.LevenbergMarquardt(res, 3, pmin, pmax, scale).start(starts)
    whole = make().run(6)
    parts = make().run(2).run(4)
    for key in ('theta', 'cost', 'lam', 'A', 'g', 'pgrad', 'trial'):
        assert same_bits(host(getattr(whole, key)), host(getattr(parts, key))), key
    for key in ('status', 'niter', 'picked', 'unfinished'):
        assert np.array_equal(host(getattr(whole, key)), host(getattr(parts, key))), key
    # run_until reads back the one counter and nothing else
    lm = make()
    reads = []
    for method in ('item', 'cpu', 'tolist', 'numpy', '__bool__', '__int__', '__float__'):
        original = getattr(torch.Tensor, method)

        def spy(self, *a, _original=original, _method=method, **k):
            if self.is_cuda:
                reads.append((_method, self.data_ptr(), tuple(self.shape)))
            return _original(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, method, spy)
    lm.run_until(check_every=4)
    monkeypatch.undo()
    assert lm.done % 4 == 0 or lm.done == lm.s.max_iter
    assert len(reads) == -(-lm.done // 4)
    assert set(reads) == {('item', lm.unfinished.data_ptr(), (1,))}
    with pytest.raises(ValueError, match='outside the bounds'):
        eng.LevenbergMarquardt(res, 3, pmin, 1.0, scale).start(starts)
    with pytest.raises(ValueError, match=r'pmax - pmin < 2 h'):
        eng.LevenbergMarquardt(res, 3, 0.0, 1e-4, scale)
    with pytest.raises(ValueError, match='start\\(\\) comes first'):
        eng.LevenbergMarquardt(res, 3, pmin, pmax, scale).run(1)
    with pytest.raises(ValueError, match='residuals must return'):
        eng.LevenbergMarquardt(lambda t: t[:, 0], 3, pmin, pmax, scale).start(starts).run(1)


# -------------------------------------------------------------------------------------------------
# Retrieval.optimize
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def emission(eng, golden):
    ret = oc.emission_retrieval(eng, golden)
    theta0 = oc.emission_starts(ret)
    return ret, theta0, ret.optimize(theta0=theta0)


def test_optimize_refuses_free_error_parameters(eng, golden):
    ret = oc.emission_retrieval(eng, golden, free_errors=True)
    theta0 = eng.dev(np.tile(ret.params[ret.ifree], (2, 1)))
    with pytest.raises(ValueError, match=r"\['err_scale_nrs2', 'err_quad_miri'\] are free"):
        ret.optimize(theta0=theta0)
    with pytest.raises(ValueError, match='are free'):
        ret.residuals(theta0)
    assert np.all(np.isfinite(host(ret.log_posterior(theta0))))


def test_optimize_end_to_end(eng, emission):
    from pyratbay_amd import optimize as po
    ret, theta0, opt = emission
    assert ret.nfree == 10 and len(ret.igauss) == 2
    theta, cost, lp = host(opt.theta), host(opt.cost), host(opt.log_posterior)
    status = host(opt.status)
    print(f'optimize: iterations {list(host(opt.niter))} status {list(status)} cost {list(cost)}')
    assert np.all(ret.inside_host(theta))
    assert np.all(status != po.RUNNING)
    lp0 = host(ret.log_posterior(eng.dev(theta0)))
    assert np.all(lp >= lp0)
    best = opt.best()
    assert best == int(np.argmax(lp)) and lp[best] > lp0[best]
    assert same_bits(lp, host(ret.log_posterior(opt.theta)))
    assert np.array_equal(opt.bestp(), ret.expand_host(theta[best:best + 1])[0])
    assert len(opt.bestp()) == ret.npar
    # Retrieval.residuals against residuals_host on the same band fluxes (the bound of
    # test_residuals_against_the_host_statement)
    R = host(ret.residuals(opt.theta))
    flux = host(ret.bandflux(opt.theta))
    Rh = ret.residuals_host(theta, flux)
    assert R.shape == (8, 3 + 2) and np.all(np.isfinite(R))
    split, obs = ret.split_host(theta), ret.observation
    for s in range(8):
        u = obs.scale_errors_host(split['err_pars'][s])
        d = obs.offset_data_host(split['offsets'][s])
        mag = np.abs(obs.data_host) + np.abs(d - obs.data_host) + np.abs(flux[s])
        assert np.all(np.abs(R[s, :3] - Rh[s, :3]) <= EPS * (2 * mag / u + 8 * np.abs(Rh[s, :3])))
        assert np.array_equal(bits(R[s, 3:]), bits(Rh[s, 3:]))
    # the host-driven loop over the same residuals from the same starts
    want = po.lm_host(lambda t: host(ret.residuals(eng.dev(t))), theta0, ret.pmin[ret.ifree],
                      ret.pmax[ret.ifree], ret.pstep[ret.ifree])
    print(f'host-driven: iterations {list(want.niter)} status {list(want.status)} cost '
          f'{list(want.cost)}')
    gap = oc.gap_bounds(np.min(cost), np.min(want.cost))
    assert abs(np.min(cost) - np.min(want.cost)) <= gap
    # three bands and two priors for nine parameters: underdetermined
    singular, cov = host(opt.singular), host(opt.covariance)
    active = host(opt.active)
    assert np.all(singular == 1)
    for s in range(8):
        f = np.where(active[s] == 0)[0]
        assert np.all(np.isnan(cov[s][np.ix_(f, f)]))


def test_optimize_determined(eng, emission):
    """Three free parameters, the others fixed, noise-free data made at a known vector.  With
    three broad bands the three parameters must each have a band to be measured by: T_irr (all
    bands; the second one alone fixes it) and the two offsets (the first and the third band).
    T_irr, log_H2O and R_planet, the first choice, trade off against each other in emission
    (temperature, abundance and radius all scale the flux): that variant is determined on paper
    only.  Measured there: FTOL after 3 - 4 iterations at costs of 9e-11 to 5e-9, 13 K, 0.13 dex
    and 1.3e-3 R_jup from the known vector: the damped steps along the valley gain less than
    ftol max(cost, 1) = 1e-10 each, which is FTOL's criterion as stated, not cost <= ftol."""
    ret0 = emission[0]
    free = ('T_irr', 'offset_nrs1', 'offset_miri')
    rows = []
    for i, name in enumerate(ret0.pnames):
        if name in free:
            rows.append([name] + [repr(float(v)) for v in (
                ret0.params[i], ret0.pmin[i], ret0.pmax[i], ret0.pstep[i])])
        else:
            rows.append([name, repr(float(ret0.constant[i]))])
    block = '\n'.join('  '.join(r) for r in rows)
    probe = eng.Retrieval(ret0.model, ret0.atmosphere, ret0.bands, ret0.observation, block,
                          chunk=2)
    truth = probe.params[probe.ifree][None, :]
    flux = host(probe.bandflux(eng.dev(truth)))[0]
    obs0 = ret0.observation
    obs = eng.Observation(flux, 0.03 * flux, ['nrs1', 'nrs2', 'miri'], obs0.offset_models,
                          obs0.err_models, units='ppm')
    ret = eng.Retrieval(ret0.model, ret0.atmosphere, ret0.bands, obs, block, chunk=2)
    rng = np.random.default_rng(9)
    theta0 = truth + 0.5 * ret.pstep[ret.ifree] * rng.uniform(-1, 1, (8, 3))
    opt = ret.optimize(theta0=theta0)
    cost, theta = host(opt.cost), host(opt.theta)
    print(f'determined: iterations {list(host(opt.niter))} status {list(host(opt.status))} cost '
          f'{list(cost)} error {np.max(np.abs(theta - truth), axis=0)}')
    assert np.all(cost <= 1e-10)
    assert np.all(host(opt.singular) == 0) and not host(opt.active).any()
    cov = host(opt.covariance)
    for s in range(8):
        assert np.all(np.isfinite(cov[s])) and np.array_equal(bits(cov[s]), bits(cov[s].T))
        assert np.all(np.linalg.eigvalsh(cov[s]) > 0)
