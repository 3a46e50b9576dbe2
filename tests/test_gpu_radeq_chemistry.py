"""Radiative equilibrium with the equilibrium chemistry of every iteration, on the device:
pb_radeq_equilibrium (csrc/pb_chemistry.hip) at its boundary -- cold against pb_equilibrium_vmr
bit for bit, warm against ChemNetwork.equilibrium_host, the fallback, a cell without a solution --
pb_radeq_update[_convective] with temps_only, and RadiativeEquilibrium(chemistry=...) on the cases
of fixture G31 (tests/golden/make_golden_radeq_chemistry.py) with both settings of
chemistry_start.  Every output buffer is pre-filled with NaN or a sentinel.

Bounds.  mm against np.sum(vmr * mass): 1e-14 relative (64 terms of one sign, each sum rounded
once: the butterfly and NumPy differ by a few ulp).  VMRs against equilibrium_host from the cold
start: 2e-12 relative wherever the host VMR is >= 1e-250, test_radeq_chemistry_cpu.py's bound for
warm against cold.  Iteration counts of a warm solve: the host warm form's +- 1.  Temperatures of a
trajectory: the fixture's max(10 s, 1e-12), s its measured sensitivity; signs, wobbling layers and
convective flags exactly.  Every check prints its figure before it asserts; the figures measured on
an MI355X are in profiles/radeq_chemistry.md."""
import numpy as np
import pytest

import chemistry_cases as cc
import radeq_cases as rc
import radeq_chemistry_cases as rq

pytestmark = pytest.mark.gpu
SENTINEL = -77
VMR_BOUND = 2e-12
DTS = [0.0, 1.0, -10.0, 50.0, -300.0, 1500.0]


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def ch():
    from pyratbay_amd import chemistry
    return chemistry


@pytest.fixture(scope='module')
def net():
    return rq.network()


def host(t):
    return t.cpu().numpy()


def carried(eng, ch, network, nw, pressure, mass, params=None, **columns):
    """A CarriedEquilibrium on buffers pre-filled with NaN (its own fill) and a status sentinel."""
    ce = ch.CarriedEquilibrium(network, nw, eng.dev(pressure), mass,
                               None if params is None else eng.dev(params), **columns)
    ce.status.fill_(SENTINEL)
    return ce


def solve(eng, ce, temps, warm):
    import torch
    ce.solve(eng.dev(np.ascontiguousarray(temps, float)), warm)
    torch.cuda.synchronize()
    return {k: host(getattr(ce, k)).copy() for k in ('vmr', 'mm', 'ln_ni', 'ln_n', 'status',
                                                     'failures')}


def deviation(vmr, want):
    seen = want >= 1e-250
    return np.where(seen, np.abs(vmr / np.where(seen, want, 1.0) - 1.0), 0.0).max()


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# The three networks of the boundary tests: (S, E) = (2, 1), (16, 5), (32, 8)
def networks(ch):
    return {'hydrogen': (cc.hydrogen_network(ch), np.array(cc.MASS[:2]), None, {}),
            'chno': (cc.network(ch), np.array(cc.MASS),
                     np.array([[0.0, cc.B[2] / cc.B[4]], [1.0, 0.6], [-1.0, 1.2]]),
                     dict(par_metal=0, ratios=[(2, 4, 1)])),
            'padded': (cc.padded_network(ch, 32), np.linspace(1.0, 60.0, 32), None, {})}


def grid(nw, L):
    """pressure[L] and temps[nw, L] inside every network's Gibbs table."""
    pressure = np.logspace(-6, 1, L) if L > 1 else np.array([0.1])
    temps = 900.0 + 350.0 * np.arange(nw * L).reshape(nw, L) % 2900.0
    return pressure, temps


# --------------------------------------------------------------------------- kernel boundary
@pytest.mark.parametrize('shape', [(3, 5), (1, 1)])
@pytest.mark.parametrize('which', ['hydrogen', 'chno', 'padded'])
def test_cold_launch_has_the_bits_of_pb_equilibrium_vmr(eng, ch, which, shape):
    import torch
    network, mass, params, columns = networks(ch)[which]
    nw, L = shape
    pressure, temps = grid(nw, L)
    params = None if params is None else params[:nw]
    ce = carried(eng, ch, network, nw, pressure, mass, params, **columns)
    got = solve(eng, ce, temps, warm=False)
    want_vmr, want_status = ch.equilibrium_vmr(
        network, eng.dev(temps), eng.dev(pressure),
        None if params is None else eng.dev(params), **columns)
    torch.cuda.synchronize()
    assert np.all(got['status'] > 0), got['status']
    assert np.array_equal(got['status'], host(want_status))
    assert np.array_equal(got['vmr'], host(want_vmr))
    mm = np.sum(got['vmr'] * mass, axis=-1)
    err = np.max(np.abs(got['mm'] / mm - 1.0))
    # the stored iterate: ln n_i of these VMRs
    ni = np.exp(got['ln_ni'])
    back = deviation(ni / ni.sum(axis=-1, keepdims=True), got['vmr'])
    print(f'{which} {shape}: iterations {got["status"].min()}-{got["status"].max()}, mm '
          f'{err:.2e} (1e-14), iterate -> VMR {back:.2e} (1e-13)')
    assert err <= 1e-14
    assert np.all(np.isfinite(got['ln_ni'])) and np.all(np.isfinite(got['ln_n']))
    assert back <= 1e-13
    assert not got['failures'].any()


@pytest.fixture(scope='module')
def warm_case(eng, ch, net):
    """15 cells of the 16-species network: a cold launch at T, then a warm launch at T + dT with
    dT per cell from DTS; the host's cold and warm solves of the same cells."""
    network, mass, params, columns = networks(ch)['chno']
    pressure, temps = grid(3, 5)
    dts = np.array(DTS)[np.arange(15) % len(DTS)].reshape(3, 5)
    ce = carried(eng, ch, network, 3, pressure, mass, params, **columns)
    first = solve(eng, ce, temps, warm=False)
    second = solve(eng, ce, temps + dts, warm=True)
    want = dict(cold=[], warm=[])
    for w in range(3):
        b = network.element_abundances_host(params[w, 0], None, {'C/O': params[w, 1]})
        start = network.equilibrium_host(temps[w], pressure, b, start='cold')[3]
        want['cold'].append(network.equilibrium_host(temps[w] + dts[w], pressure, b, start='cold'))
        want['warm'].append(network.equilibrium_host(temps[w] + dts[w], pressure, b, start=start))
    return dict(pressure=pressure, temps=temps, dts=dts, mass=mass, params=params,
                columns=columns, first=first, second=second, want=want)


def test_warm_launch(warm_case):
    got = warm_case['second']
    assert np.all(got['status'] > 0) and not got['failures'].any()
    cold_vmr = np.array([v[0] for v in warm_case['want']['cold']])
    cold_its = np.array([v[1] for v in warm_case['want']['cold']])
    warm_its = np.array([v[1] for v in warm_case['want']['warm']])
    dev = deviation(got['vmr'], cold_vmr)
    for dt in DTS:
        pick = warm_case['dts'] == dt
        print(f'dT = {dt:6g} K: device {got["status"][pick].tolist()}, host warm '
              f'{warm_its[pick].tolist()}, host cold {cold_its[pick].tolist()}')
    print(f'warm launch against the host cold solve: {dev:.2e} (bound {VMR_BOUND:.0e})')
    assert dev <= VMR_BOUND
    assert np.all(np.abs(got['status'] - warm_its) <= 1)
    mm = np.sum(got['vmr'] * warm_case['mass'], axis=-1)
    assert np.max(np.abs(got['mm'] / mm - 1.0)) <= 1e-14
    # at dT = 0 the stored solution is the solution: the fewest iterations a solve can take
    assert got['status'][warm_case['dts'] == 0.0].max() <= 2


def test_fallback_to_the_cold_start(eng, ch, warm_case):
    """Two cells with a NaN in the stored iterate, one with +700 everywhere (finite; nothing
    converges from it): bit for bit the cold launch; the others as in the warm test."""
    import torch
    c = warm_case
    network = networks(ch)['chno'][0]
    ce = carried(eng, ch, network, 3, c['pressure'], c['mass'], c['params'], **c['columns'])
    solve(eng, ce, c['temps'], warm=False)
    ce.ln_ni[0, 1, 3] = float('nan')
    ce.ln_n[1, 4] = float('nan')
    ce.ln_ni[2, 2] = 700.0
    got = solve(eng, ce, c['temps'] + c['dts'], warm=True)
    cold = carried(eng, ch, network, 3, c['pressure'], c['mass'], c['params'], **c['columns'])
    want = solve(eng, cold, c['temps'] + c['dts'], warm=False)
    torch.cuda.synchronize()
    damaged = np.zeros((3, 5), bool)
    damaged[0, 1] = damaged[1, 4] = damaged[2, 2] = True
    for k in ('vmr', 'mm', 'ln_ni', 'ln_n', 'status'):
        assert np.array_equal(got[k][damaged], want[k][damaged]), k
        assert np.array_equal(got[k][~damaged], c['second'][k][~damaged]), k
    assert not got['failures'].any()
    print(f'fallback: statuses {got["status"][damaged].tolist()} (cold '
          f'{want["status"][damaged].tolist()})')


@pytest.mark.parametrize('warm', [False, True])
def test_a_cell_without_a_solution_keeps_what_it_had(eng, ch, warm_case, warm):
    """max_iterations = 3 (no cell converges, neither way), and with the default a temperature
    above the Gibbs table, at 0 and NaN: the status, + 1 in failures, nothing else written."""
    c = warm_case
    network = networks(ch)['chno'][0]
    ce = carried(eng, ch, network, 3, c['pressure'], c['mass'], c['params'], **c['columns'])
    if warm:
        solve(eng, ce, c['temps'], warm=False)
        ce.status.fill_(SENTINEL)
    before = {k: host(getattr(ce, k)).copy() for k in ('vmr', 'mm', 'ln_ni', 'ln_n')}
    ce.model.max_iterations = 3
    got = solve(eng, ce, c['temps'] + 300.0, warm=warm)
    assert np.all(got['status'] == ch.STATUS_NOT_CONVERGED)
    assert np.all(got['failures'] == 1)
    assert same({k: got[k] for k in before}, before)
    ce.model.max_iterations = ch.MAX_ITERATIONS
    temps = c['temps'].copy()
    temps[0, 2], temps[1, 0], temps[2, 4] = 7000.0, 0.0, np.nan
    got = solve(eng, ce, temps, warm=warm)
    bad = np.zeros((3, 5), bool)
    bad[0, 2] = bad[1, 0] = bad[2, 4] = True
    assert got['status'][0, 2] == ch.STATUS_TEMPERATURE
    assert got['status'][1, 0] == got['status'][2, 4] == ch.STATUS_REJECTED
    assert np.all(got['status'][~bad] > 0)
    assert np.array_equal(got['failures'], 1 + bad)
    for k in before:
        assert np.array_equal(got[k][bad], before[k][bad], equal_nan=True), k
        assert np.all(np.isfinite(got[k][~bad])), k


def test_entry_refusals(eng, ch, net):
    from pyratbay_amd import _capi
    pressure, temps = grid(3, 5)
    with pytest.raises(ValueError, match='hybrid'):
        ch.CarriedEquilibrium(net, 3, eng.dev(pressure), cc.MASS, hybrids=[(3, 0)])
    with pytest.raises(ValueError, match='mol_mass'):
        ch.CarriedEquilibrium(net, 3, eng.dev(pressure), cc.MASS[:5])
    ce = carried(eng, ch, net, 3, pressure, cc.MASS)
    with pytest.raises(ValueError, match='temps must be'):
        ce.solve(eng.dev(temps[:2]), False)
    ce.model.nhybrid = 1
    with pytest.raises(_capi.PbError, match='hybrid'):
        ce.solve(eng.dev(temps), False)
    ce.model.nhybrid = 0
    ce.state.tol_all = 0.0
    with pytest.raises(_capi.PbError, match='tol_all'):
        ce.solve(eng.dev(temps), True)
    assert bool((ce.status == SENTINEL).all())


# -------------------------------------------------------------------------------- temps_only
def with_temps_only(monkeypatch, update, *args):
    """update(*args) (an update_on_device of the radeq test helpers) with pb_radeq.temps_only set
    on the struct it passes."""
    from pyratbay_amd import _capi
    real = _capi.call

    def call(name, state, *rest):
        state._obj.temps_only = 1
        return real(name, state, *rest)
    with monkeypatch.context() as m:
        m.setattr(_capi, 'call', call)
        return update(*args)


ATMOSPHERE = ('dens', 'cdens', 'radius', 'intervals')


@pytest.mark.parametrize('L', [2, 9, 70, 300])
def test_update_temps_only(eng, monkeypatch, L):
    import test_gpu_radeq_update as tru
    s = tru.state(L, 3, 'hydro_m', per_profile_vmr=True)
    full = rc.update_on_device(eng, s)
    only = with_temps_only(monkeypatch, rc.update_on_device, eng, s)
    for k in full:
        if k in ATMOSPHERE:
            assert np.all(np.isnan(only[k])) and not np.any(np.isnan(full[k])), k
        else:
            assert np.array_equal(only[k], full[k], equal_nan=True), k
    assert np.all(np.isfinite(only['temps'][:, -1])) and np.all(only['iter'] == 4)
    # init_only takes no notice of temps_only: the atmosphere of temp_d
    init = with_temps_only(monkeypatch, rc.update_on_device, eng, s, True)
    want = rc.update_on_device(eng, s, True)
    for k in ATMOSPHERE:
        assert np.array_equal(init[k], want[k]) and not np.any(np.isnan(init[k])), k


@pytest.mark.parametrize('L', [2, 9, 70, 300])
def test_update_convective_temps_only(eng, monkeypatch, L):
    import radeq_convection_cases as rcc
    import test_gpu_radeq_convection as trc
    s = trc.state(L, 5)
    full = rcc.update_on_device(eng, s)
    only = with_temps_only(monkeypatch, rcc.update_on_device, eng, s)
    for k in full:
        if k == 'radius':                              # (an input here: as it was on entry)
            assert np.array_equal(only[k], s['radius']), k
        elif k in ATMOSPHERE:
            assert np.all(np.isnan(only[k])), k
        else:
            assert np.array_equal(only[k], full[k], equal_nan=True), k
    assert np.all(np.isfinite(only['conv_flux'])) and np.all(only['convective'] >= 0)
    print(f'L = {L}: convective {only["convective"].tolist()}')


# ------------------------------------------------------------------------------ trajectories
def bound(name):
    return max(10.0 * float(rq.fixture()[f'{name}_sens']), 1e-12)


_RUNS = {}


def full_run(eng, name, start):
    """The case's 8 iterations with diagnostics, once per (case, chemistry_start)."""
    if (name, start) not in _RUNS:
        c = rq.case(name)
        _, re = rq.build(eng, c, chemistry_start=start)
        temps = host(re.run(c['temp0'], rq.NITER, diagnostics=True, convection=c['convection']))
        _RUNS[name, start] = (re, temps, {k: host(v) for k, v in re.history.items()})
    return _RUNS[name, start]


@pytest.mark.parametrize('start', ['previous', 'cold'])
@pytest.mark.parametrize('name', rq.CASES)
def test_trajectory(eng, net, name, start):
    c, fx = rq.case(name), rq.fixture()
    re, temps, hist = full_run(eng, name, start)
    want = fx[f'{name}_temps']
    assert temps.shape == want.shape == (c['nw'], rq.NITER + 1, c['L'])
    assert np.array_equal(temps[:, 0], c['temp0'])
    assert hist['vmr'].shape == (c['nw'], rq.NITER, c['L'], len(rq.SPECIES))
    assert hist['chem_iterations'].shape == (c['nw'], rq.NITER, c['L'])
    for w in range(c['nw']):
        terr = np.max(np.abs(temps[w] - want[w]) / want[w])
        dF = np.diff(hist['q_up'][w] - hist['q_down'][w], axis=1, prepend=np.nan)
        if c['convection']:
            used = hist['q_up'][w] - hist['q_down'][w] + hist['conv_flux'][w]
            dF = np.where(hist['convective'][w][:, None] != 0, np.diff(used, axis=1,
                                                                       prepend=np.nan), dF)
            assert np.array_equal(hist['convective'][w] != 0, fx[f'{name}_convective'][w])
        dF[:, 0] = 0.0
        assert np.array_equal(np.sign(dF), fx[f'{name}_sign'][w]), w
        assert np.array_equal(hist['wobble'][w] != 0, fx[f'{name}_wobble'][w]), w
        b = rq.abundances(c, w)
        last = net.equilibrium_host(temps[w, -1], c['pressure'], b, start='cold')[0]
        verr = deviation(host(re.vmr)[w], last)
        mm = np.sum(host(re.vmr)[w] * c['mol_mass'], axis=-1)
        merr = np.max(np.abs(host(re.mean_mass)[w] / mm - 1.0))
        its = hist['chem_iterations'][w]
        print(f'case {name} profile {w}, {start}: temperatures {terr:.2e} (bound '
              f'{bound(name):.2e}), .vmr against the host at the last row {verr:.2e} (bound '
              f'{VMR_BOUND:.0e}), mean mass {merr:.2e}, solver iterations {its.min()}-'
              f'{its.max()} (mean {its.mean():.2f})')
        assert terr <= bound(name)
        assert verr <= VMR_BOUND and merr <= 1e-14
    assert not host(re.chem_failures).any()
    assert np.array_equal(host(re.vmr), hist['vmr'][:, -1])
    assert np.array_equal(host(re.chem_status), hist['chem_iterations'][:, -1])
    assert np.all(hist['chem_iterations'] > 0)


@pytest.mark.parametrize('name', rq.CASES)
def test_previous_start_takes_fewer_iterations(eng, name):
    warm = full_run(eng, name, 'previous')[2]['chem_iterations']
    cold = full_run(eng, name, 'cold')[2]['chem_iterations']
    print(f'case {name}: solver iterations after iteration 0, previous {warm[:, 1:].sum()} '
          f'({warm[:, 1:].min()}-{warm[:, 1:].max()}), cold {cold[:, 1:].sum()} '
          f'({cold[:, 1:].min()}-{cold[:, 1:].max()})')
    assert np.all(warm[:, 1:] <= cold[:, 1:])
    assert warm[:, 1:].sum() < cold[:, 1:].sum()


def test_batch_equals_its_profiles_one_at_a_time(eng):
    """Case (q), three profiles with their own [M/H], C/O and start, chemistry_start='cold': bit
    for bit."""
    import torch
    c = rq.case('q')
    re, temps, hist = full_run(eng, 'q', 'cold')
    for w in range(c['nw']):
        _, one = rq.build(eng, c, w=w, chemistry_start='cold')
        t1 = one.run(c['temp0'][w], rq.NITER)
        assert tuple(t1.shape) == (1, rq.NITER + 1, c['L'])
        assert np.array_equal(host(t1)[0], temps[w]), w
        assert torch.equal(one.vmr[0], re.vmr[w]) and torch.equal(one.mean_mass[0], re.mean_mass[w])
        assert torch.equal(one.chem_status[0], re.chem_status[w])
        assert torch.equal(one.radius[0], re.radius[w])


def test_continue_run(eng):
    """4 + 4 iterations with continue_run on case (r) against the host chain restarted the same
    way (the stored iterate, VMRs and dt_scale kept, a fresh sign history)."""
    c, fx = rq.case('r'), rq.fixture()
    half = rq.NITER // 2
    _, re = rq.build(eng, c)
    first = host(re.run(c['temp0'], half, convection=True))
    second = host(re.run(nsamples=half, continue_run=True, diagnostics=True, convection=True))
    assert np.array_equal(second[:, 0], first[:, -1])
    got = np.concatenate([first[0], second[0, 1:]])
    want = fx['r_restart_temps']
    tol = max(10.0 * float(fx['r_restart_sens']), 1e-12)
    err = np.max(np.abs(got - want) / want)
    dts = fx['r_restart_dt_scale'][half:]
    derr = np.max(np.abs(host(re.history['dt_scale'])[0] - dts) / dts)
    its = host(re.history['chem_iterations'])
    print(f'continue_run: temperatures {err:.2e} (bound {tol:.2e}), dt_scale {derr:.2e}; solver '
          f'iterations of the first continued step {its[0, 0].min()}-{its[0, 0].max()}')
    assert err <= tol and derr <= 1e-12
    assert not np.allclose(got, fx['r_temps'][0], rtol=1e-6, atol=0)
    assert not host(re.chem_failures).any()
    # the iterate was kept: the first solve after the restart is a warm one
    cold = rq.network().equilibrium_host(second[0, 1], c['pressure'], rq.abundances(c, 0),
                                         start='cold')[1]
    assert np.all(its[0, 0] <= cold) and its[0, 0].sum() < cold.sum()


def test_loop_is_launches_only(eng):
    """The loop with chemistry allocates nothing and waits for nothing: the allocator's counters
    do not move between a run and its repetition, but for the history it returns."""
    import torch
    c = rq.case('p')
    _, re = rq.build(eng, c)
    re.run(c['temp0'], 2)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    re.run(c['temp0'], 6)
    mid = torch.cuda.memory_stats()['allocation.all.allocated']
    re.run(c['temp0'], 12)
    after = torch.cuda.memory_stats()['allocation.all.allocated']
    assert after - mid == mid - before


def test_refusals(eng, net, monkeypatch):
    """ValueError before any launch: no entry of the library has been called."""
    from pyratbay_amd import _capi, radeq
    c = rq.case('p')
    model, _ = rq.build(eng, c)

    def no_call(name, *args):
        raise AssertionError(f'{name} called')
    monkeypatch.setattr(_capi, 'call', no_call)
    monkeypatch.setattr(radeq._capi, 'call', no_call)

    def make(vmr=None, **kw):
        args = dict(tint=float(c['tint'][0]), flux_top=c['flux_top'][0], tmin=c['tmin'],
                    tmax=c['tmax'], table_species=rq.TABLE_SPECIES, chemistry=net,
                    metallicity=0.0, e_ratio={'C/O': 0.55})
        args.update(kw)
        return radeq.RadiativeEquilibrium(model, c['pressure'], vmr, c['mol_mass'], **args)

    def refused(match, temp0=None, **kw):
        with pytest.raises(ValueError, match=match):
            re = make(**kw)
            if temp0 is not None:
                re.run(temp0, 2)
    refused('vmr must be None', vmr=np.full((c['L'], 16), 1.0 / 16))
    refused('table species SO2 is not in species', table_species=['H2O', 'CO', 'SO2'])
    refused("species are the network's", species=rc.SPECIES)
    refused('profile 0: an element ratio <= 0', e_ratio={'C/O': 0.0})
    refused('profile 1: an element ratio <= 0', e_ratio={'C/O': np.array([0.5, -1.0, 0.6])})
    refused('profile 2: .*not finite', metallicity=np.array([0.0, 0.1, np.nan]))
    refused("is not in the network", e_scale={'Fe': 0.1})
    refused("chemistry_start 'x'", chemistry_start='x')
    refused('abundances of chemistry=', chemistry=None, vmr=np.full((c['L'], 16), 1.0 / 16),
            species=rq.SPECIES)
    refused('range of the Gibbs table', temp0=np.full(c['L'], 150.0), tmin=100.0)
    # the default range is cut to the Gibbs table's as well as the opacity table's
    re = make(tmin=None, tmax=None)
    assert re.tmin == max(float(model.tmin), net.gibbs_temps[0])
    assert re.tmax == min(float(model.tmax), net.gibbs_temps[-1])
