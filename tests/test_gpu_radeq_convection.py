"""The convective radiative-equilibrium update (k_radeq_update<true> behind
pb_radeq_update_convective, csrc/pb_radeq.hip) and RadiativeEquilibrium.run(convection=True).

At the kernel boundary, test_gpu_radeq_update.py's method: hand-made parts and state, every output
pre-filled with NaN / -1, against radeq.step_convective_host and the host atmosphere.  Qup, Qdown,
the sign row, the wobbling layers and the convective flag bit for bit; temperatures, dt_scale,
densities, radius and intervals to 1e-12; conv_flux within max(10 S, 1e-12), S being the largest
relative change of the host statement's conv_flux when the temperatures it is evaluated at are
multiplied by 1 + 1e-15 r (r uniform in [-1, 1], seeded): the device's log, pow and sqrt are an
ulp off libm's, 10x is the margin for that.  Three profiles per launch, steps of milli-kelvin
(dt_scale from 2 to 6), so that the profile the flux is evaluated at keeps the start's shape:
  0  temperature falling with depth: convects nowhere; its bottom layers lie below tmin and are
     clipped onto it, which is a node of the heat-capacity table;
  1  T ~ p**0.25 against grad_ad around 0.12 (cp / R from 7.5 to 9): convects in every layer below
     the isothermal top (layers 0 and 1; with 2 layers that is the whole profile); from 70 layers
     on its bottom lies above the table's last node;
  2  falling with depth but for a jump of 30 % in the middle: convects in a few layers.
|grad_t - grad_ad| >= 1e-2 at every layer >= 1 is asserted on the host statement.

End to end: the four cases of fixture G26 (tests/golden/make_golden_radeq_convection.py) within
max(10 sens, 1e-12) of the trajectories the reference's own loop recorded with convection=True."""
import numpy as np
import pytest

import radeq_cases as rc
import radeq_convection_cases as cc

pytestmark = pytest.mark.gpu

RTOL = 1e-12
TMIN, TMAX = 300.0, 3500.0
CP_TEMPS = np.array([300.0, 500.0, 800.0, 1200.0, 1800.0, 2500.0])
CP_TABLE = np.stack([7.5 + 1.5 * (CP_TEMPS - 300.0) / 2200.0 + 0.1 * s for s in range(4)], axis=1)
MPLANET = 0.6 * 1.8982e30
RADIUS = {
    2: dict(radius_model=None),
    3: dict(radius_model='hydro_g', gravity=2200.0, p0=1.0, r0=7.1492e9),
    9: dict(radius_model='hydro_m', mplanet=MPLANET, p0=1.0, r0=7.1492e9),
    70: dict(radius_model='hydro_g', gravity=2200.0, p0=1.0, r0=7.1492e9),
    300: dict(radius_model='hydro_m', mplanet=MPLANET, p0=1.0, r0=7.1492e9),
}


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def state(L, P):
    """The state of the module docstring: L layers, P parts, k = 6 previous sign rows (the window
    of four, wrapped) with 5 parts and 1 with one."""
    from pyratbay_amd import radeq
    rng = np.random.default_rng(1000 * L + P)
    nw, k = 3, (6 if P == 5 else 1)
    # four decades up to 100 bar, at most eight layers per decade
    step = min(0.125, 4.0 / (L - 1))
    pressure = 100.0 * 10.0**(-step * np.arange(L - 1, -1, -1))
    x = np.log(pressure / pressure[0]) / np.log(1e4)          # 0 at the top; 1 four decades below
    mid = L // 2
    jump = np.where(np.arange(L) >= max(mid, 2), 1.3, 1.0)
    temp = np.array([330.0 - 50.0 * np.linspace(0.0, 1.0, L),
                     320.0 * (pressure / pressure[0])**0.25,
                     1000.0 * np.exp(-0.1 * x) * jump])
    kw = dict(RADIUS[L])
    if kw.get('p0') is not None:
        kw['p0'] = float(np.sqrt(pressure[L // 2] * pressure[L // 2 - 1]))
    qdown = 1e7 * (1.0 + rng.uniform(0, 1, (nw, L)))
    qup = qdown + 3e5 * rng.uniform(-1, 1, (nw, L))
    q = np.stack([qup, qdown], axis=1)
    if P == 1:
        parts = q[:, None]
    else:
        split = rng.uniform(0.1, 0.2, (nw, P - 1, 2, L))
        first = split * q[:, None]
        parts = np.concatenate([first, (q - np.sum(first, axis=1))[:, None]], axis=1)
    vmr = np.tile([0.85, 0.1494, 4e-4, 2e-4], (L, 1)) * (1 + 0.1 * x[:, None])
    s = dict(parts=np.ascontiguousarray(parts), temp=temp,
             dt_scale=rng.uniform(2.0, 6.0, (nw, L)),
             signs=rng.integers(-1, 2, (nw, k, L)).astype(float), pressure=pressure, vmr=vmr,
             tab_map=[2, 3], cont_map=[0, 1, 0], tmin=TMIN, tmax=TMAX, radius_kwargs=kw,
             cp_temps=CP_TEMPS, cp_table=CP_TABLE, mplanet=MPLANET, alpha=1.5, beta=0.5)
    # the radius on entry: that of the evaluated profile (a hydrostatic one for the fixed model too)
    hydro = kw if kw['radius_model'] else RADIUS[3] | dict(p0=kw.get('p0') or float(pressure[-1]))
    s['radius'] = np.array([radeq.atmosphere_host(temp[w], pressure, vmr, np.array(rc.MASS),
                                                  **hydro)[1] for w in range(nw)])
    return s


@pytest.mark.parametrize('P', [1, 5])
@pytest.mark.parametrize('L', [2, 3, 9, 70, 300])
def test_update_convective(eng, L, P):
    from pyratbay_amd import radeq
    s = state(L, P)
    k = s['signs'].shape[1]
    got = cc.update_on_device(eng, s)
    rng = np.random.default_rng(7)
    layers = []
    for w in range(3):
        want = cc.update_on_host(s, w)
        first = want['radiative']
        # the inputs are what the docstring says: no layer near the switch
        table = radeq.heat_capacity_host(CP_TEMPS, CP_TABLE, first['temp'])
        cp_over_r = np.sum(table * s['vmr'], axis=1)
        grad_ad = 1.0 - (cp_over_r - 1.0) / cp_over_r
        grad_t = np.ediff1d(np.log(first['temp']), to_begin=0.0) / \
            np.ediff1d(np.log(s['pressure'] * 1e6), to_begin=1.0)
        assert np.min(np.abs(grad_t - grad_ad)[1:]) >= 1e-2, (w, np.abs(grad_t - grad_ad)[1:].min())
        assert np.all(np.isfinite(want['conv_flux'])) and np.all(want['conv_flux'] >= 0.0)
        layers.append(int(np.sum(want['conv_flux'] > 0.0)))
        # bit for bit
        assert np.array_equal(got['q_up'][w], want['q_up'])
        assert np.array_equal(got['q_down'][w], want['q_down'])
        assert np.array_equal(got['signs'][w, k % 4], want['sign'])
        assert np.array_equal(got['wobble'][w], want['wobble'].astype(np.int32))
        assert got['convective'][w] == int(want['convective'])
        for it in range(max(k - 3, 0), k):                   # the other rows of the ring stay
            assert np.array_equal(got['signs'][w, it % 4], s['signs'][w, it])
        # conv_flux within ten times its sensitivity to the last bits of the temperatures
        sens = 0.0
        live = want['conv_flux'] > 0.0
        for _ in range(4):
            other = cc.update_on_host(s, w, 1.0 + 1e-15 * rng.uniform(-1, 1, L))['conv_flux']
            assert np.array_equal(other > 0.0, live)
            if live.any():
                sens = max(sens, np.max(np.abs(other[live] / want['conv_flux'][live] - 1.0)))
        bound = max(10.0 * sens, 1e-12)
        assert np.all(got['conv_flux'][w][~live] == 0.0)
        err = np.max(np.abs(got['conv_flux'][w][live] / want['conv_flux'][live] - 1.0)) \
            if live.any() else 0.0
        print(f'L {L} parts {P} profile {w}: {layers[-1]} convecting layers, conv_flux {err:.2e} '
              f'(bound {bound:.2e})')
        assert err <= bound
        np.testing.assert_allclose(got['dt_scale'][w], want['dt_scale'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got['temps'][w, k + 1], want['temp'], rtol=RTOL, atol=0)
        assert np.array_equal(got['temp'][w], got['temps'][w, k + 1])
        assert np.all(np.isnan(got['temps'][w, :k + 1]))
        assert got['iter'][w] == k + 1
        assert abs(got['sigma'][w] - want['sigma']) <= 1e-12
        np.testing.assert_allclose(got['dens'][w], want['dens'][:, s['tab_map']], rtol=RTOL)
        np.testing.assert_allclose(got['cdens'][w], want['dens'][:, s['cont_map']], rtol=RTOL)
        if s['radius_kwargs']['radius_model'] is None:
            assert np.array_equal(got['radius'][w], s['radius'][w])          # (not touched)
            assert np.all(np.isnan(got['intervals']))
        else:
            np.testing.assert_allclose(got['radius'][w], want['radius'], rtol=RTOL, atol=0)
            np.testing.assert_allclose(got['intervals'][w], -np.diff(want['radius']), rtol=RTOL,
                                       atol=0)
        if w == 0:
            # clipped onto tmin = the table's first node; the radiative result stands
            assert first['temp'][-1] == TMIN == CP_TEMPS[0]
            assert np.array_equal(want['temp'], first['temp'])
        if w == 1 and L >= 70:
            assert first['temp'][-1] > CP_TEMPS[-1]                           # outside the table
        if w == 1 and L > 2:
            assert not np.array_equal(want['sign'], first['sign']) or \
                not np.array_equal(want['temp'], first['temp'])
    # what the states were made for
    if L == 2:
        assert layers == [0, 0, 0]                   # the isothermal top is the whole profile
    else:
        assert layers[0] == 0 and layers[1] == L - 2 and 1 <= layers[2] < max(L - 2, 3)
        assert list(got['convective']) == [0, 1, 1]


def stiff_table():
    return cc.CP_TEMPS, cc.cp_table('stiff')


def test_same_bits_as_the_radiative_loop_where_nothing_convects(eng):
    """cp / R = 1.05 (grad_ad = 0.95): run(convection=True) is run(convection=False) bit for bit,
    on case (b) of G26 (which does convect with its own table) and the three profiles of (d)."""
    import torch
    for name in ('b', 'd'):
        c = cc.case(name)
        _, plain = cc.build(eng, c, heat_capacity=stiff_table())
        want = plain.run(c['temp0'], cc.NITER, diagnostics=True)
        want_hist, want_dts = plain.history, plain.dt_scale.clone()
        _, conv = cc.build(eng, c, heat_capacity=stiff_table())
        got = conv.run(c['temp0'], cc.NITER, diagnostics=True, convection=True)
        assert not conv.history['convective'].any()
        assert torch.equal(conv.history['conv_flux'], torch.zeros_like(conv.history['conv_flux']))
        assert torch.equal(got, want) and torch.equal(conv.dt_scale, want_dts)
        for key in ('q_up', 'q_down', 'dt_scale', 'wobble', 'sigma'):
            assert torch.equal(conv.history[key], want_hist[key]), key
        assert plain.conv_flux is None and 'conv_flux' not in want_hist


_RUNS = {}


def full_run(eng, name):
    if name not in _RUNS:
        c = cc.case(name)
        _, re = cc.build(eng, c)
        temps = host(re.run(c['temp0'], cc.NITER, diagnostics=True, convection=True))
        _RUNS[name] = (re, temps, {k: host(v) for k, v in re.history.items()})
    return _RUNS[name]


@pytest.mark.parametrize('name', cc.CASES)
def test_trajectory(eng, name):
    """The whole batch of a case in one call against the reference's recorded trajectory."""
    c, fx = cc.case(name), cc.fixture()
    re, temps, hist = full_run(eng, name)
    want_t, want_dts = fx[f'{name}_temps'], fx[f'{name}_dt_scale']
    assert temps.shape == want_t.shape == (c['nw'], cc.NITER + 1, c['L'])
    assert hist['conv_flux'].shape == (c['nw'], cc.NITER, c['L'])
    assert hist['convective'].shape == (c['nw'], cc.NITER)
    tol = max(10.0 * float(fx[f'{name}_sens']), 1e-12)
    assert np.array_equal(hist['convective'], fx[f'{name}_convective'].astype(np.int32))
    for w in range(c['nw']):
        terr = np.max(np.abs(temps[w] - want_t[w]) / want_t[w])
        derr = np.max(np.abs(hist['dt_scale'][w] - want_dts[w]) / want_dts[w])
        want_f = fx[f'{name}_conv_flux'][w]
        assert np.array_equal(hist['conv_flux'][w] != 0.0, want_f != 0.0)
        live = want_f != 0.0
        got_f = hist['conv_flux'][w]
        ferr = np.max(np.abs(got_f[live] / want_f[live] - 1.0)) if live.any() else 0.0
        print(f'case {name} profile {w}: temperatures {terr:.2e} (bound {tol:.2e}), dt_scale '
              f'{derr:.2e}, conv_flux {ferr:.2e} (reported)')
        assert terr <= tol
        assert derr <= 1e-12                 # (exact signs: the same factors and filter)
    assert np.array_equal(host(re.conv_flux), hist['conv_flux'][:, -1])
    assert np.array_equal(host(re.convective), hist['convective'][:, -1])
    assert np.array_equal(host(re.dt_scale), hist['dt_scale'][:, -1])


def test_continue_run(eng):
    """4 + 4 iterations of case (c) against the host statements chained the same way (a fresh sign
    history at the restart, the loop's own dt_scale kept) on the device's own fluxes: within the
    end-to-end bound of the case."""
    from pyratbay_amd import radeq
    c, fx = cc.case('c'), cc.fixture()
    half = cc.NITER // 2
    _, re = cc.build(eng, c)
    first = host(re.run(c['temp0'], half, diagnostics=True, convection=True))
    hists = [{k: host(v) for k, v in re.history.items()}]
    second = host(re.run(nsamples=half, continue_run=True, diagnostics=True, convection=True))
    hists.append({k: host(v) for k, v in re.history.items()})
    assert np.array_equal(second[:, 0], first[:, -1])
    got = np.concatenate([first[0], second[0, 1:]])
    tol = max(10.0 * float(fx['c_sens']), 1e-12)
    temp, dts = c['temp0'][0], np.full(c['L'], radeq.DT_SCALE0)
    for k in range(cc.NITER):
        h, i = hists[k // half], k % half
        signs = np.zeros((0, c['L'])) if i == 0 else np.vstack([signs, s['sign']])
        assert np.max(np.abs(got[k] - temp) / temp) <= tol
        s = cc.host_step(c, 0, temp, dts, signs, h['q_up'][0, i], h['q_down'][0, i])
        assert h['convective'][0, i] == int(s['convective'])
        assert np.array_equal(h['wobble'][0, i], s['wobble'].astype(np.int32))
        np.testing.assert_allclose(h['dt_scale'][0, i], s['dt_scale'], rtol=1e-12, atol=0)
        temp, dts = s['temp'], s['dt_scale']
    assert np.max(np.abs(got[-1] - temp) / temp) <= tol
    # the restart shows: the straight run of the fixture goes elsewhere
    assert not np.allclose(got, fx['c_temps'][0], rtol=1e-6, atol=0)
    assert not hists[1]['wobble'][0, 0].any()


def test_refusals(eng, monkeypatch):
    """ValueError before any launch: no entry of the library has been called."""
    from pyratbay_amd import _capi, radeq

    def no_call(name, *args):
        raise AssertionError(f'{name} called')
    c = cc.case('b')
    table = (c['cp_temps'], c['cp_table'][0])
    model, plain = rc.build(eng, c)
    monkeypatch.setattr(_capi, 'call', no_call)
    monkeypatch.setattr(radeq._capi, 'call', no_call)

    def make(**kw):
        args = dict(tint=float(c['tint'][0]), flux_top=c['flux_top'][0], tmin=c['tmin'],
                    tmax=c['tmax'], species=rc.SPECIES, table_species=rc.TABLE_SPECIES,
                    heat_capacity=table, mplanet=c['mplanet'])
        args.update(kw)
        return radeq.RadiativeEquilibrium(model, c['pressure'], c['vmr'], c['mol_mass'], **args)

    def refused(match, run=True, **kw):
        with pytest.raises(ValueError, match=match):
            re = make(**kw)
            if run:
                re.run(c['temp0'], 2, convection=True)
    refused('needs the heat capacities', heat_capacity=None)
    refused('needs mplanet > 0', mplanet=None)
    refused('needs mplanet > 0', mplanet=0.0)
    refused('got shapes', run=False, heat_capacity=(table[0], table[1][:, :3]))
    refused('got shapes', run=False, heat_capacity=(table[0][:-1], table[1]))
    refused('ascending', run=False, heat_capacity=(table[0][::-1].copy(), table[1]))
    bad = table[1].copy()
    bad[3, 1] = np.nan
    refused('not finite', run=False, heat_capacity=(table[0], bad))
    bad[3, 1] = 1.0
    refused('cp_over_R <= 1', run=False, heat_capacity=(table[0], bad))
    refused('different numbers of profiles', run=False, tint=np.ones(2),
            heat_capacity=(table[0], np.array([table[1]] * 3)))
    refused('hydro_g needs p0 and r0', radius_model='hydro_g', gravity=2200.0)
    refused('mixing_length', run=False, mixing_length=(1.5, -0.5))
