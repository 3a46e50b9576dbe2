"""What test_observation_cpu.py and test_gpu_observation.py share: fixture G25
(tests/golden/make_golden_observation.py) in the forms the package takes, and seeded cases."""
import numpy as np


def observation_of(g, module):
    """G25's data with its offset and error models -> module.Observation."""
    return module.Observation(g['data'], g['uncert'], [str(n) for n in g['band_names']],
                              [str(m) for m in g['offset_models']],
                              [str(m) for m in g['err_models']], units=str(g['units']))


def star_bands(g):
    """G25's pass bands in the form engine.PassBands takes: (first grid index, response on the
    band's samples -- the wavelength factor of a photon-counting band folded in --, height)."""
    wn = g['star_wn']
    out = []
    for b in range(int(g['star_nbands'])):
        idx, response = g[f'star_band{b}_idx'], g[f'star_band{b}_response']
        assert np.all(np.diff(idx) == 1)
        if bool(g[f'star_band{b}_counting']):
            response = response * (1.0 / (wn[idx] * 1.0e-4))
        out.append((int(idx[0]), response, float(g[f'star_band{b}_height'])))
    return out


def random_observation(module, nb, noff, nerr, seed, units='ppm'):
    """nb data points over max(noff, nerr, 1) instruments dealt round-robin, the first noff of
    them with an offset model and the first nerr with an error model of alternating mode."""
    rng = np.random.default_rng(seed)
    ninst = max(noff, nerr, 1)
    names = [f'inst{b % ninst}x' for b in range(nb)]
    # (fewer points than instruments: only the models that still match a point)
    noff, nerr = min(noff, nb), min(nerr, nb)
    data = rng.uniform(1e-3, 2e-3, nb)
    uncert = rng.uniform(1e-5, 5e-5, nb)
    offs = [f'offset_inst{j}x' for j in range(noff)]
    errs = [('err_scale_' if j % 2 == 0 else 'err_quad_') + f'inst{j}x' for j in range(nerr)]
    return module.Observation(data, uncert, names, offs, errs, units=units)


def random_pars(obs, nw, seed):
    """(models[nw, nb], offsets[nw, noff] or None, err_pars[nw, nerr] or None) around obs."""
    rng = np.random.default_rng(seed)
    models = obs.data_host[None, :] * (1 + rng.normal(0, 0.02, (nw, obs.nbands)))
    offsets = rng.uniform(-300.0, 300.0, (nw, obs.noff)) if obs.noff else None
    err_pars = None
    if obs.nerr:
        err_pars = np.where(obs.err_mode_host[None, :] == 0, rng.uniform(-0.3, 0.5, (nw, obs.nerr)),
                            rng.uniform(0.5, 2.5, (nw, obs.nerr)))
    return models, offsets, err_pars


BAND_COUNTS = [2, 3, 255, 256, 257, 600]       # samples per band: the block of 256 lanes' edges


def star_case(nt, nw, W=700, seed=0):
    """A smooth positive SED grid[nt, W], one band per BAND_COUNTS on W samples (random
    responses and heights), and nw stellar temperatures inside the grid with its first node, its
    last node and an inner node among them (as far as nw allows)."""
    rng = np.random.default_rng(1000 * nt + nw + seed)
    wn = 1850.0 + np.cumsum(rng.uniform(0.8, 1.6, W))
    sed_temps = np.sort(rng.uniform(3500.0, 7000.0, nt))
    x = np.linspace(0.0, 1.0, W)
    fluxes = (1.0e5 * (sed_temps[:, None] / 5000.0)**3.5 * (1 + 0.3 * x[None, :]) *
              (1 + 0.05 * np.sin(9.0 * x[None, :] + sed_temps[:, None] / 900.0)))
    bands = []
    for count in BAND_COUNTS:
        start = int(rng.integers(0, W - count + 1))
        bands.append((start, rng.uniform(0.1, 1.0, count), float(rng.uniform(0.5, 2.0))))
    tstar = rng.uniform(sed_temps[0], sed_temps[-1], nw)
    tstar[0] = sed_temps[0]
    if nw > 1:
        tstar[-1] = sed_temps[-1]
    if nw > 2:
        tstar[1] = sed_temps[nt // 2]
    planet = rng.uniform(1e3, 5e3, (nw, W))
    return dict(wn=wn, sed_temps=sed_temps, fluxes=fluxes, bands=bands, tstar=tstar,
                planet=planet, rstar=8.8e10, rplanet=7.1e9,
                rplanets=7.1e9 * rng.uniform(0.8, 1.3, nw),
                f_dilution=rng.uniform(0.5, 1.0, nw))
