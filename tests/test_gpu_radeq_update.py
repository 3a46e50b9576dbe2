"""The radiative-equilibrium update (k_radeq_update behind pb_radeq_update, csrc/pb_radeq.hip) on
hand-made parts and state, against radeq.step_host and the host atmosphere
(radeq.atmosphere_host): the signs of dF and the wobbling layers exactly; dt_scale, the new
temperatures, densities, radius and intervals to 1e-12 (the device's pow is an ulp off libm's:
profiles/clouds.md; everything else is the same IEEE operations in the same order).

Three profiles with a state each:
  0  dt_scale = 1: steps of micro-kelvin, the temperature filter's sigma on its lower clip (0.75);
     layer 2 (layer 1 when L = 2) repeats the fluxes of the layer above: dF is exactly 0 there;
  1  dt_scale = 1e8 and dF > 0 in every layer: sigma on its upper clip (2.0), every layer pushed
     onto tmax;
  2  dt_scale = 1e8 and dF < 0: every layer onto tmin; from L = 5 on, dt_scale around 2e5 with
     random signs instead (temperatures inside their clips; with the full sign window, where
     most layers wobble, sigma lies between its clips).
The sign history is random (-1, 0, 1), k rows of it: k = 0 (nothing wobbles), 3 (a partial
window), 6 (the window of four, and the ring of four rows has wrapped).  L = 2, 3, 5 lie below
every filter radius (3 ... 8: the reflected extension repeats), L = 65 is past a wavefront.  The
isothermal top is set BEFORE the temperature filter, which then mixes layers 0 and 1 differently,
so it shows in the comparison with step_host, not as temp[0] == temp[1]."""
import numpy as np
import pytest

import radeq_cases as rc

pytestmark = pytest.mark.gpu

RTOL = 1e-12
TMIN, TMAX = 250.0, 3000.0
RADIUS = {
    None: dict(radius_model=None),
    'hydro_g': dict(radius_model='hydro_g', gravity=2200.0, p0=1.0, r0=7.1492e9),
    'hydro_g0': dict(radius_model='hydro_g', gravity=2200.0, p0=None, r0=None),
    'hydro_m': dict(radius_model='hydro_m', mplanet=0.6 * 1.8982e30, p0=1.0, r0=7.1492e9),
}


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def state(L, k, radius, per_profile_vmr=False):
    rng = np.random.default_rng(100 * L + k)
    nw, P = 3, 3
    x = np.linspace(0.0, 1.0, L)
    # eight layers per decade up to 100 bar whatever L is (dpress = 0.29: the steps of profiles 1
    # and 2 are hundreds of kelvin even at L = 2); the reference pressure lies inside the grid
    pressure = 100.0 * 10.0**(-0.125 * np.arange(L - 1, -1, -1))
    kw = dict(RADIUS[radius])
    if kw.get('p0') is not None:
        kw['p0'] = float(np.sqrt(pressure[L // 2] * pressure[L // 2 - 1]))
    # Qup - Qdown rising (profile 1), falling (profile 2) or flat + noise (profile 0) with depth
    qdown = 1e7 * (1.0 + rng.uniform(0, 1, (nw, L)))
    qnet = np.array([3e5 * rng.uniform(-1, 1, L), 1e6 * (1 + x) + 1e4 * np.arange(L),
                     -1e6 * (1 + x) - 1e4 * np.arange(L)])
    dt_scale = np.array([np.ones(L), np.full(L, 1e8), np.full(L, 1e8)])
    # (profiles 1 and 2 start within a kelvin of the bound they are pushed onto)
    temp = np.array([rng.uniform(900.0, 1800.0, L), TMAX - rng.uniform(0.1, 1.0, L),
                     TMIN + rng.uniform(0.1, 1.0, L)])
    if L >= 5:
        qnet[2] = 3e5 * rng.uniform(-1, 1, L)
        dt_scale[2] = 2e5 * rng.uniform(0.5, 1.5, L)
        temp[2] = rng.uniform(900.0, 1800.0, L)
    qup = qdown + qnet
    split = rng.uniform(0.2, 0.4, (nw, 2, 2, L))
    q = np.stack([qup, qdown], axis=1)                       # [nw, 2, L]
    parts = np.stack([split[:, 0] * q, split[:, 1] * q,
                      q - split[:, 0] * q - split[:, 1] * q], axis=1)
    same = min(2, L - 1)
    parts[0, :, :, same] = parts[0, :, :, same - 1]          # dF = 0 exactly
    signs = rng.integers(-1, 2, (nw, k, L)).astype(float)
    vmr = np.tile([0.85, 0.1494, 4e-4, 2e-4], (L, 1)) * (1 + 0.1 * x[:, None])
    if per_profile_vmr:
        vmr = np.array([vmr, vmr * 0.9, vmr * 1.05])
    return dict(parts=np.ascontiguousarray(parts), temp=temp, dt_scale=dt_scale, signs=signs,
                pressure=pressure, vmr=vmr, tab_map=[2, 3], cont_map=[0, 1, 0],
                tmin=TMIN, tmax=TMAX, radius_kwargs=kw)


@pytest.mark.parametrize('radius', list(RADIUS))
@pytest.mark.parametrize('k', [0, 3, 6])
@pytest.mark.parametrize('L', [2, 3, 5, 65])
def test_update(eng, L, k, radius):
    s = state(L, k, radius, per_profile_vmr=(k == 3))
    got = rc.update_on_device(eng, s)
    sigmas = []
    for w in range(3):
        want = rc.update_on_host(s, w)
        assert np.array_equal(got['q_up'][w], want['q_up'])
        assert np.array_equal(got['q_down'][w], want['q_down'])
        assert np.array_equal(got['signs'][w, k % 4], want['sign'])
        assert np.array_equal(got['wobble'][w], want['wobble'].astype(np.int32))
        if k == 0:
            assert not got['wobble'][w].any()
        np.testing.assert_allclose(got['dt_scale'][w], want['dt_scale'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got['temps'][w, k + 1], want['temp'], rtol=RTOL, atol=0)
        assert np.array_equal(got['temp'][w], got['temps'][w, k + 1])
        assert np.all(np.isnan(got['temps'][w, :k + 1]))              # (only row k + 1)
        assert got['iter'][w] == k + 1
        # the other rows of the ring stay
        for it in range(max(k - 3, 0), k):
            assert np.array_equal(got['signs'][w, it % 4], s['signs'][w, it])
        np.testing.assert_allclose(got['dens'][w], want['dens'][:, s['tab_map']], rtol=RTOL)
        np.testing.assert_allclose(got['cdens'][w], want['dens'][:, s['cont_map']], rtol=RTOL)
        if radius is None:
            assert np.all(np.isnan(got['radius'])) and np.all(np.isnan(got['intervals']))
        else:
            assert np.all(np.isfinite(want['radius']))
            np.testing.assert_allclose(got['radius'][w], want['radius'], rtol=RTOL, atol=0)
            np.testing.assert_allclose(got['intervals'][w], -np.diff(want['radius']), rtol=RTOL,
                                       atol=0)
        assert abs(got['sigma'][w] - want['sigma']) <= 1e-12
        sigmas.append(want['sigma'])
    # what the states were made for
    same = min(2, L - 1)
    assert got['signs'][0, k % 4, same] == 0.0 and got['signs'][0, k % 4, 0] == 0.0
    assert got['sigma'][0] == 0.75 and got['sigma'][1] == 2.0
    assert np.all(got['temp'][1] == TMAX)
    if L >= 5:
        if k == 6:
            assert 0.75 < sigmas[2] < 2.0            # (a data-dependent filter radius)
        assert np.all((got['temp'][2] > TMIN) & (got['temp'][2] < TMAX))
    else:
        assert np.all(got['temp'][2] == TMIN)


@pytest.mark.parametrize('L', [257, 300, 744, 1023, 1024])
def test_more_layers_than_threads(eng, L):
    """Above the 256 threads of the workgroup every thread owns several layers, the parts are
    added by ONE group whose sums lie over two of the profile's rows in LDS, and the mean of
    |dT| is NumPy's pairwise sum four halvings deep (1023: a block of 135 after three).  744 is
    the most the net-flux kernel takes, 1024 the most this one does."""
    s = state(L, 6, 'hydro_g')
    got = rc.update_on_device(eng, s)
    for w in range(3):
        want = rc.update_on_host(s, w)
        assert np.array_equal(got['q_up'][w], want['q_up'])
        assert np.array_equal(got['q_down'][w], want['q_down'])
        assert np.array_equal(got['signs'][w, 6 % 4], want['sign'])
        assert np.array_equal(got['wobble'][w], want['wobble'].astype(np.int32))
        np.testing.assert_allclose(got['dt_scale'][w], want['dt_scale'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got['temps'][w, 7], want['temp'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got['dens'][w], want['dens'][:, s['tab_map']], rtol=RTOL)
        np.testing.assert_allclose(got['radius'][w], want['radius'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got['intervals'][w], -np.diff(want['radius']), rtol=RTOL,
                                   atol=0)
        assert abs(got['sigma'][w] - want['sigma']) <= 1e-12


def test_init_only(eng):
    """init_only: the atmosphere of temp_d and nothing else."""
    import ctypes as C
    L, k = 65, 2
    s = state(L, k, 'hydro_m', per_profile_vmr=True)
    got = rc.update_on_device(eng, s, init_only=True)
    from pyratbay_amd import radeq
    for w in range(3):
        dens, radius = radeq.atmosphere_host(s['temp'][w], s['pressure'], s['vmr'][w],
                                             np.array(rc.MASS), **s['radius_kwargs'])
        np.testing.assert_allclose(got['dens'][w], dens[:, s['tab_map']], rtol=RTOL)
        np.testing.assert_allclose(got['cdens'][w], dens[:, s['cont_map']], rtol=RTOL)
        np.testing.assert_allclose(got['radius'][w], radius, rtol=RTOL)
        np.testing.assert_allclose(got['intervals'][w], -np.diff(radius), rtol=RTOL)
    assert np.all(got['iter'] == k) and np.all(np.isnan(got['temps']))
    assert np.all(np.isnan(got['q_up'])) and np.all(got['wobble'] == -1)
    assert np.array_equal(got['temp'], s['temp']) and np.array_equal(got['dt_scale'], s['dt_scale'])
    assert C.sizeof(radeq.RadeqStruct) % 8 == 0


def test_sign_window_is_four_rows(eng):
    """A sign that differed five iterations ago does not wobble; four ago it does."""
    L = 5
    for k, old, wobbles in ((5, 0, False), (5, 1, True), (4, 0, True)):
        s = state(L, k, None)
        qup, qdown = rc.sum_parts(s['parts'])
        now = np.sign(np.ediff1d(qup[2] - qdown[2], to_begin=0))
        s['signs'][2] = now                                  # profile 2 never changed sign ...
        s['signs'][2, old, 3] = -now[3] if now[3] else 1.0   # ... but for layer 3, at iteration `old`
        got = rc.update_on_device(eng, s)
        want = rc.update_on_host(s, 2)
        assert bool(want['wobble'][3]) == wobbles
        assert np.array_equal(got['wobble'][2], want['wobble'].astype(np.int32))
        assert got['wobble'][2].sum() == int(wobbles)
