"""RadiativeEquilibrium.run (pyratbay_amd/radeq.py: interpolation, pb_two_stream_net_batch,
pb_radeq_update per iteration, nothing read back) on the five cases of fixture G23 against the
trajectories the reference's own radiative_equilibrium recorded (tests/golden/make_golden_radeq.py):
the signs of dF and the wobbling layers of every iteration exactly, Qup and Qdown of the first
iteration to 1e-12 of their maximum, and the temperatures of every iteration within the case's
sensitivity bound.

The bound is not chosen here: the generator ran the reference chain a second time with Qup and
Qdown perturbed by 1e-12 (relative, uniform, seeded) and stored the largest relative temperature
deviation s over the 8 iterations; a run may deviate by 10 s (the kernel's error need not be
uniform), but no less than 1e-12 is asked.  test_radeq_cpu.py shows the fixture's preconditions.

Worst deviations measured on an MI355X are in profiles/radeq.md."""
import numpy as np
import pytest

import radeq_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def bound(name):
    return max(10.0 * float(rc.fixture()[f'{name}_sens']), 1e-12)


_RUNS = {}


def full_run(eng, name):
    """The case's 8 iterations with diagnostics, once per case: (object, temps, history)."""
    if name not in _RUNS:
        c = rc.case(name)
        # (case d leaves tmin / tmax to their defaults: the table's range cut by the CIA tables')
        _, re = rc.build(eng, c, **(dict(tmin=None, tmax=None) if name == 'd' else {}))
        temps = host(re.run(c['temp0'], rc.NITER, diagnostics=True))
        _RUNS[name] = (re, temps, {k: host(v) for k, v in re.history.items()})
    return _RUNS[name]


def reference_steps(c, w):
    """The wobbling layers and sigmas of the recorded trajectory, from step_host on its rows."""
    from pyratbay_amd import radeq
    fx, name = rc.fixture(), c['name']
    dpress = radeq.log_pressure_steps(c['pressure'])
    signs, out = np.zeros((0, c['L'])), []
    for k in range(rc.NITER):
        dts = fx[f'{name}_dt_scale'][w, k - 1] if k else np.full(c['L'], radeq.DT_SCALE0)
        s = radeq.step_host(fx[f'{name}_temps'][w, k], dts, signs, fx[f'{name}_qup'][w, k],
                            fx[f'{name}_qdown'][w, k], dpress, c['tmin'], c['tmax'])
        signs = np.vstack([signs, s['sign']])
        out.append(s)
    return out


@pytest.mark.parametrize('name', rc.CASES)
def test_trajectory(eng, name):
    c, fx = rc.case(name), rc.fixture()
    re, temps, hist = full_run(eng, name)
    want_t, want_dts = fx[f'{name}_temps'], fx[f'{name}_dt_scale']
    qup, qdown = fx[f'{name}_qup'], fx[f'{name}_qdown']
    assert temps.shape == want_t.shape == (c['nw'], rc.NITER + 1, c['L'])
    assert np.array_equal(temps[:, 0], c['temp0'])
    tol = bound(name)
    assert (re.tmin, re.tmax) == (c['tmin'], c['tmax'])
    if name == 'd':
        cia = re.model.continuum.cia
        assert re.tmin == max([float(re.model.tmin)] + [float(m.tmin) for m in cia])
        assert re.tmax == min([float(re.model.tmax)] + [float(m.tmax) for m in cia])
    for w in range(c['nw']):
        steps = reference_steps(c, w)
        for k in range(rc.NITER):
            dF = np.ediff1d(hist['q_up'][w, k] - hist['q_down'][w, k], to_begin=0)
            assert np.array_equal(np.sign(dF), steps[k]['sign']), (w, k)
            assert np.array_equal(hist['wobble'][w, k], steps[k]['wobble'].astype(np.int32)), (w, k)
        scale = max(qup[w, 0].max(), qdown[w, 0].max())
        qerr = max(np.abs(hist['q_up'][w, 0] - qup[w, 0]).max(),
                   np.abs(hist['q_down'][w, 0] - qdown[w, 0]).max()) / scale
        terr = np.max(np.abs(temps[w] - want_t[w]) / want_t[w])
        derr = np.max(np.abs(hist['dt_scale'][w] - want_dts[w]) / want_dts[w])
        print(f'case {name} profile {w}: Q of iteration 0 {qerr:.2e} (1e-12), temperatures '
              f'{terr:.2e} (bound {tol:.2e}), dt_scale {derr:.2e}')
        assert qerr <= 1e-12
        assert terr <= tol
        assert derr <= 1e-12                 # (exact signs: the same factors and filter)
    # what run() leaves behind
    assert np.array_equal(host(re.temps), temps)
    assert np.array_equal(host(re.dt_scale), hist['dt_scale'][:, -1])
    assert np.array_equal(host(re.q_up), hist['q_up'][:, -1])
    assert np.array_equal(host(re.q_down), hist['q_down'][:, -1])
    assert tuple(re.spectrum.shape) == (c['nw'], c['W'])


def test_continue_run(eng):
    """4 + 4 iterations with continue_run on case (c) against the reference's function called
    twice (the second time with radeq_temps = atleast_2d(last row) and the dt_scale it left).  Most
    layers wobble across the restart, so the restarted trajectory differs from the straight one by
    2e-2 (test_radeq_cpu.py): a continue_run that kept the sign rows, or a reset dt_scale, fails.
    The bound is the restarted trajectory's own sensitivity, measured like every case's."""
    from pyratbay_amd import radeq
    c, fx = rc.case('c'), rc.fixture()
    half = rc.NITER // 2
    _, re = rc.build(eng, c)
    first = host(re.run(c['temp0'], half))
    second = host(re.run(nsamples=half, continue_run=True, diagnostics=True))
    assert np.array_equal(second[:, 0], first[:, -1])
    got = np.concatenate([first[0], second[0, 1:]])
    want, want_dts = fx['c_restart_temps'], fx['c_restart_dt_scale']
    tol = max(10.0 * float(fx['c_restart_sens']), 1e-12)
    err = np.max(np.abs(got - want) / want)
    derr = np.max(np.abs(host(re.history['dt_scale'])[0] - want_dts[half:]) / want_dts[half:])
    print(f'continue_run: temperatures {err:.2e} (bound {tol:.2e}), dt_scale {derr:.2e}')
    assert err <= tol and derr <= 1e-12
    # the wobbling layers after the restart: none at once, then against the rows since the restart
    dpress = radeq.log_pressure_steps(c['pressure'])
    signs = np.zeros((0, c['L']))
    for k in range(half, rc.NITER):
        s = radeq.step_host(want[k], want_dts[k - 1], signs, fx['c_restart_qup'][k],
                            fx['c_restart_qdown'][k], dpress, c['tmin'], c['tmax'])
        signs = np.vstack([signs, s['sign']])
        assert np.array_equal(host(re.history['wobble'])[0, k - half], s['wobble'].astype(np.int32))
    assert not host(re.history['wobble'])[0, 0].any()
    assert not np.allclose(got, fx['c_temps'][0], rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match='not from a temp0'):
        re.run(c['temp0'], half, continue_run=True)


def test_batch_equals_its_profiles_one_at_a_time(eng):
    """Case (e), three profiles with their own tint, flux_top and start: bit for bit."""
    import torch
    c = rc.case('e')
    re, temps, hist = full_run(eng, 'e')
    for w in range(c['nw']):
        _, one = rc.build(eng, c, tint=float(c['tint'][w]), flux_top=c['flux_top'][w])
        t1 = one.run(c['temp0'][w], rc.NITER)
        assert tuple(t1.shape) == (1, rc.NITER + 1, c['L'])
        assert np.array_equal(host(t1)[0], temps[w]), w
        assert torch.equal(one.spectrum[0], re.spectrum[w])
        assert torch.equal(one.q_up[0], re.q_up[w]) and torch.equal(one.dt_scale[0], re.dt_scale[w])
    # and a second run of the batch gives the same bits
    _, again = rc.build(eng, c)
    assert np.array_equal(host(again.run(c['temp0'], rc.NITER)), temps)


@pytest.mark.parametrize('name', ['b', 'c'])
def test_spectrum_is_eval_at_the_last_evaluated_profile(eng, name):
    """.spectrum = flux_up[0] at temps[-2], against the one-profile eval() there (1e-11 of the
    column's largest flux, the bound of test_gpu_two_stream_batch.py: eval() interpolates with
    another kernel); Qup, Qdown against torch.trapezoid of eval()'s flux arrays likewise."""
    import torch
    import test_gpu_two_stream_batch as tsb
    c = rc.case(name)
    re, temps, hist = full_run(eng, name)
    model = re.model
    last = temps[0, -2]
    dens, radius = rc.host_atmosphere(c, last)
    model.set_radius(radius)
    itab = [rc.SPECIES.index(s) for s in rc.TABLE_SPECIES]
    want = host(model.eval(last, np.ascontiguousarray(dens[:, itab])))
    up, down = host(model.flux_up), host(model.flux_down)
    tsb.close_by_column(host(re.spectrum)[0], want, tsb.RTOL, np.max(np.abs(up), axis=0))
    wn = eng.dev(c['wn'])
    qup = host(torch.trapezoid(model.flux_up, wn, dim=1))
    qdown = host(torch.trapezoid(model.flux_down, wn, dim=1))
    scale = max(qup.max(), qdown.max())
    assert np.abs(host(re.q_up)[0] - qup).max() <= 1e-11 * scale
    assert np.abs(host(re.q_down)[0] - qdown).max() <= 1e-11 * scale


def test_temp0_decides_the_number_of_profiles_when_all_inputs_are_shared(eng):
    """Shared vmr, tint and flux_top: a [L] temp0 runs one profile, a [3, L] temp0 three, run by
    run on the same object, and every row equals the one-profile run from that start; with a
    per-profile input the number is fixed and another one refused."""
    c = rc.case('b')
    _, re = rc.build(eng, c)
    one = host(re.run(c['temp0'][0], 3))
    starts = np.array([c['temp0'][0], c['temp0'][0] - 50.0, c['temp0'][0] + 30.0])
    three = host(re.run(starts, 3))
    assert one.shape == (1, 4, c['L']) and three.shape == (3, 4, c['L'])
    assert np.array_equal(three[0], one[0])
    again = host(re.run(starts[2], 3))
    assert again.shape == (1, 4, c['L']) and np.array_equal(again[0], three[2])
    e = rc.case('e')
    _, fixed = rc.build(eng, e)
    with pytest.raises(ValueError, match='temp0 has 2 profiles, the model 3'):
        fixed.run(e['temp0'][:2], 2)
    assert tuple(fixed.run(e['temp0'][0], 2).shape) == (3, 3, e['L'])


def test_loop_is_launches_only(eng):
    """The loop allocates nothing and waits for nothing: the allocator's counters do not move
    between a run and its repetition on the same object, but for the history it returns."""
    import torch
    c = rc.case('b')
    _, re = rc.build(eng, c)
    re.run(c['temp0'], 2)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    re.run(c['temp0'], 6)
    mid = torch.cuda.memory_stats()['allocation.all.allocated']
    re.run(c['temp0'], 12)
    after = torch.cuda.memory_stats()['allocation.all.allocated']
    assert after - mid == mid - before          # (the same few set-up allocations, not 6 more steps')
