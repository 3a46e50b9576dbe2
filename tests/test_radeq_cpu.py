"""CPU-only checks of the radiative-equilibrium loop (pyratbay_amd/radeq.py, csrc/pb_radeq.hip):
the entries are exported and check their arguments before any HIP call, RadiativeEquilibrium
refuses what it cannot run before any launch, step_host reproduces the rows the reference's own
loop recorded (fixture G23, tests/golden/make_golden_radeq.py), and the fixture meets the
preconditions the GPU tests' tolerances rest on."""
import ctypes as C
import types

import numpy as np
import pytest

import radeq_cases as rc


def spectrum(L=9, W=130, S=2, rt_path='two_stream', continuum=None, tmin=200.0, tmax=3800.0):
    """What RadiativeEquilibrium reads of a TableSpectrum before it touches the device."""
    return types.SimpleNamespace(rt_path=rt_path, rt_path_name=rt_path, nlayers=L, nwave=W,
                                 nspec=S, tmin=tmin, tmax=tmax, continuum=continuum)


def continuum(**kw):
    args = dict(alkali=[], deck=[], cloud=[], cia=[], species=['H2', 'He'])
    args.update(kw)
    return types.SimpleNamespace(**args)


def make(spec=None, **kw):
    from pyratbay_amd import radeq
    spec = spectrum() if spec is None else spec
    L = spec.nlayers
    args = dict(pressure=np.logspace(-6, 2, L), vmr=np.full((L, 4), 0.25), mol_mass=rc.MASS,
                species=rc.SPECIES, table_species=rc.TABLE_SPECIES)
    args.update(kw)
    return radeq.RadiativeEquilibrium(spec, args.pop('pressure'), args.pop('vmr'),
                                      args.pop('mol_mass'), **args)


def test_symbols_exported():
    from pyratbay_amd import _capi
    for name in ('pb_two_stream_net_batch', 'pb_two_stream_net_work_doubles',
                 'pb_two_stream_net_parts', 'pb_radeq_update'):
        assert name in _capi.exported_names() and hasattr(_capi.lib(), name)
    lib = _capi.lib()
    assert lib.pb_two_stream_net_work_doubles.restype is C.c_int64
    assert [lib.pb_two_stream_net_parts(w) for w in (0, 1, 256, 257, 600)] == [0, 1, 1, 2, 3]
    assert lib.pb_two_stream_net_work_doubles(81, 100000, 512) >= 512 * 80 * 100000 > 2**31
    assert lib.pb_two_stream_net_work_doubles(1, 100, 3) == 0


def test_net_entry_checks_arguments_first():
    from pyratbay_amd import _capi
    fake = C.c_void_p(16)          # never dereferenced: the checks come first
    good = [fake, fake, fake, fake, fake, fake, fake, None, 0, None, 0, fake, 12, 100, 4, None]

    def refused(match, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        with pytest.raises(_capi.PbError, match=match):
            _capi.call('pb_two_stream_net_batch', *args)

    refused('bad shape', a12=0)
    refused('bad shape', a13=-1)
    for k in range(7):             # flux, parts, ec, intervals, wn, weights, temps
        refused('null pointer', **{f'a{k}': None})
    refused('strides', a8=7)
    refused('strides', a10=99)
    refused('null work', a11=None)
    refused('layers', a12=1 << 20)
    assert _capi.call('pb_two_stream_net_batch', *([None] * 8 + [0, None, 0, None, 12, 0, 4, None])) == 0


def test_update_entry_checks_arguments_first():
    from pyratbay_amd import _capi, radeq
    with pytest.raises(_capi.PbError, match='null state'):
        _capi.call('pb_radeq_update', None, 0, None)
    st = radeq.RadeqStruct()
    st.nwalkers = 2
    for L in (1, 1025, 100000):
        st.nlayers = L
        with pytest.raises(_capi.PbError, match=f'2-1024 layers, not {L}'):
            _capi.call('pb_radeq_update', C.byref(st), 0, None)
    st.nlayers, st.nrows = 9, 5
    with pytest.raises(_capi.PbError, match='null pointer'):
        _capi.call('pb_radeq_update', C.byref(st), 0, None)
    st.nwalkers = 0
    assert _capi.call('pb_radeq_update', C.byref(st), 0, None) == 0


def test_refusals():
    """ValueError before any launch (no GPU here: a launch would raise PbError instead)."""
    def refused(match, spec=None, run=None, **kw):
        with pytest.raises(ValueError, match=match):
            model = make(spec, **kw)
            if run is not None:
                model.run(**run)

    refused('two-stream geometry', spectrum(rt_path='emission'))
    refused('two-stream geometry', spectrum(rt_path='transit'))
    refused('alkali models', spectrum(continuum=continuum(alkali=['sodium'])))
    refused('a Deck', spectrum(continuum=continuum(deck=['deck'])))
    refused('cloud-type models', spectrum(continuum=continuum(cloud=['lecavelier'])))
    refused('at least 2', spectrum(L=1), pressure=np.array([1.0]), vmr=np.full((1, 4), 0.25))
    refused('at most 744', spectrum(L=745), pressure=np.logspace(-6, 2, 745),
            vmr=np.full((745, 4), 0.25))
    refused('pressure must have shape', pressure=np.logspace(-6, 2, 8))
    refused('ascending', pressure=np.logspace(2, -6, 9))
    refused('vmr must have shape', vmr=np.full((8, 4), 0.25))
    refused('mol_mass must have shape', mol_mass=[1.0, 2.0])
    refused('species names', species=['H2', 'He'])
    refused('not in species', table_species=['H2O', 'CH4'])
    refused('needs species', spectrum(continuum=continuum()), species=None, table_species=None)
    refused('radius_model', radius_model='hydrostatic')
    refused('gravity', radius_model='hydro_g')
    refused('mplanet', radius_model='hydro_m', p0=0.1, r0=7e9)
    refused('p0 and r0', radius_model='hydro_m', mplanet=1e30)
    refused('outside the pressure grid', radius_model='hydro_g', gravity=2200.0, p0=1e3, r0=7e9)
    refused('flux_top must have shape', flux_top=np.ones(129))
    refused('different numbers of profiles', tint=np.ones(3), flux_top=np.ones((2, 130)))
    refused('temp0 must have shape', run=dict(temp0=np.full(8, 1000.0), nsamples=2))
    refused('temp0 outside the 200.0-3800.0 K', run=dict(temp0=np.full(9, 4000.0), nsamples=2))
    refused('temp0 outside the 200.0-3800.0 K', run=dict(temp0=np.full(9, 150.0), nsamples=2))
    refused('temp0 has 2 profiles', tint=np.ones(3), run=dict(temp0=np.full((2, 9), 900.0)))
    refused('continue_run without', run=dict(continue_run=True))
    # the defaults of tmin / tmax: the table's range cut by the CIA tables'
    cia = [types.SimpleNamespace(tmin=60.0, tmax=3000.0), types.SimpleNamespace(tmin=250.0, tmax=7000.0)]
    model = make(spectrum(continuum=continuum(cia=cia)))
    assert (model.tmin, model.tmax) == (250.0, 3000.0)
    refused('outside the 250.0-3000.0 K', spectrum(continuum=continuum(cia=cia)),
            run=dict(temp0=np.full(9, 3100.0)))


def test_trapezoid_weights():
    from pyratbay_amd import radeq
    rng = np.random.default_rng(5)
    for W in (2, 3, 70, 257):
        wn = np.cumsum(rng.uniform(0.5, 2.0, W))
        y = rng.uniform(1, 2, (4, W))
        got = np.sum(radeq.trapezoid_weights(wn) * y, axis=1)
        np.testing.assert_allclose(got, np.trapezoid(y, wn, axis=1), rtol=1e-14)
    assert np.array_equal(radeq.trapezoid_weights([3.0]), [0.0])


def test_gaussian_filter_is_scipys():
    from scipy.ndimage import gaussian_filter1d
    from pyratbay_amd import radeq
    rng = np.random.default_rng(6)
    for n in (2, 3, 5, 9, 65):
        x = rng.uniform(1, 2, n)
        for sigma in (0.75, 0.874, 0.876, 1.5, 1.999, 2.0):
            assert np.array_equal(radeq.gaussian_filter1d(x, sigma), gaussian_filter1d(x, sigma))


def replay(c, w):
    """step_host along the recorded trajectory of profile w: per iteration the step's dict."""
    from pyratbay_amd import radeq
    fx = rc.fixture()
    temps, dts = fx[f'{c["name"]}_temps'][w], fx[f'{c["name"]}_dt_scale'][w]
    qup, qdown = fx[f'{c["name"]}_qup'][w], fx[f'{c["name"]}_qdown'][w]
    dpress = radeq.log_pressure_steps(c['pressure'])
    signs, out = np.zeros((0, c['L'])), []
    for k in range(rc.NITER):
        s = radeq.step_host(temps[k], dts[k - 1] if k else np.full(c['L'], radeq.DT_SCALE0),
                            signs, qup[k], qdown[k], dpress, c['tmin'], c['tmax'])
        signs = np.vstack([signs, s['sign']])
        out.append(s)
    return out


@pytest.mark.parametrize('name', rc.CASES)
def test_step_host_against_the_reference(name):
    """Every recorded iteration: the next temperatures and dt_scale to 1e-13 (the same NumPy
    statements: in practice the same bits), the signs of dF from the recorded Qup, Qdown.  The
    reference records no wobble rows: a wrong wobble set shows as a factor 0.5 / 1.15 = 0.43 in
    dt_scale."""
    c, fx = rc.case(name), rc.fixture()
    for w in range(c['nw']):
        steps = replay(c, w)
        temps, dts = fx[f'{name}_temps'][w], fx[f'{name}_dt_scale'][w]
        for k, s in enumerate(steps):
            np.testing.assert_allclose(s['temp'], temps[k + 1], rtol=1e-13, atol=0)
            np.testing.assert_allclose(s['dt_scale'], dts[k], rtol=1e-13, atol=0)
            assert np.array_equal(s['sign'], np.sign(np.ediff1d(fx[f'{name}_qup'][w, k] -
                                                                fx[f'{name}_qdown'][w, k],
                                                                to_begin=0)))
            if k == 0:
                assert not s['wobble'].any()


def test_restarted_run_is_a_fresh_sign_history():
    """c_restart: the reference's function called a second time, after 4 iterations, with the last
    row and the kept dt_scale.  step_host reproduces it with an EMPTY sign history at the restart
    and with no other: keeping the four sign rows gives other wobbling layers and another
    dt_scale.  The restarted run differs from the straight one (most layers wobble across it)."""
    from pyratbay_amd import radeq
    c, fx = rc.case('c'), rc.fixture()
    temps, dts = fx['c_restart_temps'], fx['c_restart_dt_scale']
    qup, qdown = fx['c_restart_qup'], fx['c_restart_qdown']
    assert temps.shape == (rc.NITER + 1, c['L']) and dts.shape == (rc.NITER, c['L'])
    half = rc.NITER // 2
    assert np.array_equal(temps[:half + 1], fx['c_temps'][0, :half + 1])
    assert not np.array_equal(temps[half + 1], fx['c_temps'][0, half + 1])
    assert 0.0 <= float(fx['c_restart_sens']) <= 1e-8
    dpress = radeq.log_pressure_steps(c['pressure'])
    for fresh in (True, False):
        signs, wrong = np.zeros((0, c['L'])), 0
        for k in range(rc.NITER):
            if k == half and fresh:
                signs = np.zeros((0, c['L']))
            s = radeq.step_host(temps[k], dts[k - 1] if k else np.full(c['L'], radeq.DT_SCALE0),
                                signs, qup[k], qdown[k], dpress, c['tmin'], c['tmax'])
            signs = np.vstack([signs, s['sign']])
            if fresh:
                np.testing.assert_allclose(s['temp'], temps[k + 1], rtol=1e-13, atol=0)
                np.testing.assert_allclose(s['dt_scale'], dts[k], rtol=1e-13, atol=0)
                if k == half:
                    assert not s['wobble'].any()
            else:
                wrong += not np.allclose(s['dt_scale'], dts[k], rtol=1e-6, atol=0)
        assert fresh or wrong >= 1


@pytest.mark.parametrize('name', rc.CASES)
def test_fixture_preconditions(name):
    """On the recorded reference alone: |dF| >= 1e-9 max(Qup, Qdown) at every iteration and layer
    >= 1 (below that a 1e-12 error of Q moves dF, hence dT, visibly); no temperature on a clip
    bound; the sensitivity is at most 1e-8; and in case (c) at least one layer wobbles and the
    filter's sigma takes two different values."""
    c, fx = rc.case(name), rc.fixture()
    qup, qdown, temps = fx[f'{name}_qup'], fx[f'{name}_qdown'], fx[f'{name}_temps']
    assert temps.shape == (c['nw'], rc.NITER + 1, c['L'])
    assert qup.shape == qdown.shape == (c['nw'], rc.NITER, c['L'])
    dF = np.diff(qup - qdown, axis=2)
    ratio = np.abs(dF) / np.maximum(qup, qdown)[:, :, 1:]
    print(f'case {name}: floor {ratio.min():.2e}, sensitivity {float(fx[f"{name}_sens"]):.2e}')
    assert ratio.min() >= 1e-9
    assert np.all(temps > c['tmin']) and np.all(temps < c['tmax'])
    assert 0.0 <= float(fx[f'{name}_sens']) <= 1e-8
    if name == 'c':
        steps = replay(c, 0)
        assert max(int(s['wobble'].sum()) for s in steps) >= 1
        assert len({s['sigma'] for s in steps}) >= 2
        assert min(s['sigma'] for s in steps) == 0.75 and max(s['sigma'] for s in steps) == 2.0


def test_host_chain_reproduces_the_recorded_fluxes(orc):
    """The chain of radeq_cases.host_fluxes (what the generator handed the reference as
    two_stream_rt) gives the recorded Qup, Qdown of the first iteration again."""
    for name in ('a', 'b', 'd', 'e'):
        c, fx = rc.case(name), rc.fixture()
        for w in range(c['nw']):
            down, up = rc.host_fluxes(orc, c, np.ascontiguousarray(c['temp0'][w]), w)
            assert np.array_equal(np.trapezoid(up, c['wn'], axis=1), fx[f'{name}_qup'][w, 0])
            assert np.array_equal(np.trapezoid(down, c['wn'], axis=1), fx[f'{name}_qdown'][w, 0])
