#!/usr/bin/env python3
"""Fixture G25: what the reference makes of the data and of the eclipse factor per evaluation --
instrumental offsets and uncertainty scaling (`Data.offset_data` / `Data.scale_errors`,
pyratbay/tools/data.py:210-270), the log-likelihood on the arrays they give (`Loglike.__call__`,
tools/retrieval_tools.py:74-104), and eval()'s stellar-temperature branch: the SED grid
interpolated at tstar (pyrat/argum.py:93-98), band-integrated (pyrat_obj.py:288-294) and used in
the eclipse factor (pyrat_obj.py:662-665).  Build container only:

    python tests/golden/make_golden_observation.py

The Loglike object is created without its constructor, as in make_golden_loglike.py, and given
the data and uncertainties eval() leaves in obs for each parameter row.  Only data is stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_e2e import reference_package, REF      # noqa: E402

BAND_NAMES = ['nirspec_g395h_nrs1'] * 4 + ['nirspec_g395h_nrs2'] * 4 + ['miri_lrs'] * 3
OFFSET_MODELS = ['offset_nrs2', 'offset_miri']
ERR_MODELS = ['err_scale_nrs1', 'err_quad_miri']
UNITS = 'ppm'


def main():
    if not os.path.isdir(REF):
        sys.exit('needs /root/reference')
    work = tempfile.mkdtemp(prefix='pb_obs_')
    store = {}
    try:
        reference_package(work)
        import scipy.interpolate as si
        import pyratbay.constants as pc
        import pyratbay.spectrum as ps
        from pyratbay.tools.data import Data
        from pyratbay.tools.retrieval_tools import Loglike
        rng = np.random.default_rng(25)
        # ---- offsets, error scaling and the likelihood
        nb, nrows = len(BAND_NAMES), 7
        data = rng.uniform(1e-3, 2e-3, nb)
        uncert = rng.uniform(1e-5, 5e-5, nb)
        depth = Data(data, uncert, BAND_NAMES, OFFSET_MODELS, ERR_MODELS)
        assert depth.scaling_modes == ['scale', 'quadrature']
        offsets = rng.uniform(-300.0, 300.0, (nrows, len(OFFSET_MODELS)))       # ppm
        err_pars = np.stack([rng.uniform(-0.3, 0.5, nrows),                     # log10 factor
                             rng.uniform(0.5, 2.5, nrows)], axis=1)             # log10 ppm
        offsets[2] = 0.0                        # the defaults (pyrat/observation.py:121-131)
        err_pars[2] = [0.0, -100.0]
        models = data[None, :] * (1 + rng.normal(0, 0.02, (nrows, nb)))
        models[4, 5] = np.inf                   # eval()'s reject value
        off_data = np.array([depth.offset_data(offsets[r], UNITS) for r in range(nrows)])
        sc_uncert = np.array([depth.scale_errors(err_pars[r], UNITS) for r in range(nrows)])
        models[5] = off_data[5]                 # perfect fit: the normalisation term alone
        ll = object.__new__(Loglike)
        ll.params = np.zeros(3)
        ll.ifree = np.array([0, 1, 2])
        ll.ishare = np.array([], int)
        ll.pstep = np.ones(3)
        ll._dt_snapshot = 0.0
        out = np.zeros(nrows)
        for r in range(nrows):
            ll.data, ll.uncert = off_data[r], sc_uncert[r]
            ll.func = lambda params, retmodel=False, r=r: models[r]
            out[r] = ll(np.array([0.1 * r, 0.2, 0.3]))
        assert np.array_equal(off_data[2], data) and np.array_equal(sc_uncert[2], uncert)
        assert out[4] == -1.0e98
        store.update(band_names=np.array(BAND_NAMES), offset_models=np.array(OFFSET_MODELS),
                     err_models=np.array(ERR_MODELS), units=np.array(UNITS), data=data,
                     uncert=uncert, offsets=offsets, err_pars=err_pars, models=models,
                     offset_data=off_data, scaled_uncert=sc_uncert, loglike=out,
                     unit_value=np.array(float(getattr(pc, UNITS))))
        # ---- the stellar SED grid at tstar, its band fluxes and the eclipse factor
        nwave = 700
        wn = np.linspace(1850.0, 2750.0, nwave)                 # 3.6 - 5.4 um
        sed_temps = np.array([4000.0, 4250.0, 4500.0, 5000.0, 6000.0])
        ripple = 1 + 0.05 * np.sin(np.linspace(0.0, 9.0, nwave))[None, :] * \
            np.linspace(1.0, 0.3, len(sed_temps))[:, None]
        fluxes = np.array([ps.bbflux(wn, t) for t in sed_temps]) * ripple
        assert np.all(fluxes > 0)
        bands = [ps.Tophat(4.08, 0.05, name='nrs1', wn=wn),
                 ps.Tophat(4.25, 0.07, name='nrs1', wn=wn, counting_type='energy'),
                 ps.Tophat(4.40, 0.02, name='nrs2', wn=wn),
                 ps.Tophat(4.70, 0.20, name='nrs2', wn=wn, counting_type='energy'),
                 ps.Tophat(4.95, 0.04, name='nrs2', wn=wn),
                 ps.PassBand(f'{pc.FILTERS}spitzer_irac2.dat', wn=wn)]
        tstar = np.array([4000.0, 4500.0, 6000.0, 4100.0, 4733.3, 5999.0])
        flux_interp = si.interp1d(sed_temps, fluxes, axis=0)    # pyrat/argum.py:97
        starflux = np.array([flux_interp(t) for t in tstar])
        bandflux_star = np.array([[band(s) for band in bands] for s in starflux])
        planet = rng.uniform(1e3, 5e3, (len(tstar), len(bands)))     # band(fplanet), given
        rstar = 1.27 * pc.rsun
        rplanet = np.array([1.0, 1.37]) * pc.rjup
        eclipse = np.zeros((len(rplanet),) + planet.shape)
        for j, rp in enumerate(rplanet):
            for w in range(len(tstar)):
                bandflux = np.copy(planet[w])
                rprs = rp / rstar
                bandflux *= rprs**2.0 / bandflux_star[w]          # pyrat_obj.py:664-665
                eclipse[j, w] = bandflux
        store.update(star_wn=wn, star_sed_temps=sed_temps, star_fluxes=fluxes, star_tstar=tstar,
                     star_starflux=starflux, star_bandflux_star=bandflux_star,
                     star_planet_bandflux=planet, star_rstar=np.array(rstar),
                     star_rplanet=rplanet, star_eclipse_bandflux=eclipse,
                     star_nbands=np.array(len(bands)), um=np.array(pc.um))
        for b, band in enumerate(bands):
            assert np.all(np.diff(band.idx) == 1)
            assert np.array_equal(band.wn, wn[band.idx])
            store[f'star_band{b}_idx'] = np.asarray(band.idx)
            store[f'star_band{b}_response'] = np.asarray(band.response, float)
            store[f'star_band{b}_height'] = np.array(band.height, float)
            store[f'star_band{b}_counting'] = np.array(band.counting_type == 'photon')
            store[f'star_band{b}_wl'] = np.asarray(band.wl, float)
        path = os.path.join(HERE, 'g25_observation.npz')
        np.savez_compressed(path, **store)
        print(out)
        print(os.path.getsize(path), 'bytes')
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
