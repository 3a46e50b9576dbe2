#!/usr/bin/env python3
"""Fixture G21: the high-resolution exit of eval() (pyrat/pyrat_obj.py:331-356) -- instrument
convolution, radial-velocity shift of the grid, sampling at the data.  Build container only:

    python tests/golden/make_golden_hires.py

Calls of the real package (imported as in make_golden_e2e.py): ps.inst_convolution, ps.rv_shift
and scipy.interpolate.interp1d, on ps.constant_resolution_spectrum grids for five (instrument,
sampling) resolutions and on one constant-step grid with sampling_res = None.  The taps are the
array inst_convolution hands to scipy.signal.convolve (recorded by a pass-through around that
call, which also asserts that SciPy chooses the direct method: no FFT rounding in the fixture).
Input spectra hold float32-representable values so that the archive stays small; every result
is a full double.  Only data is stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_e2e as e2e                      # noqa: E402

REF = e2e.REF
# (R_inst, R_samp); None: constant wavenumber step, sampling_res = None
CASES = [(25000.0, 123300.0), (5000.0, 123300.0), (100000.0, 300000.0), (3000.0, 30000.0),
         (1000.0, 30000.0), (20000.0, None)]
RVS = [0.0, 7.3, -31.0]
NWAVE = 2000
NDATA = 500
RADII = (1.2 * 7.1492e9, 0.9 * 6.957e10)          # rplanet, rstar (cm)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def main():
    if not os.path.isdir(REF):
        sys.exit('needs /root/reference')
    work = tempfile.mkdtemp(prefix='pb_hires_')
    store = {}
    try:
        e2e.reference_package(work)
        import pyratbay.spectrum as ps
        import pyratbay.spectrum.spec_tools as st
        import scipy
        import scipy.interpolate as si
        from scipy.signal import choose_conv_method, convolve

        taps_seen = []

        def recording_convolve(a, k, mode='full'):
            assert choose_conv_method(a, k, mode=mode) == 'direct'
            taps_seen.append(np.copy(k))
            return convolve(a, k, mode=mode)
        st.convolve = recording_convolve

        rng = np.random.default_rng(21)
        store['scipy_version'] = np.array(scipy.__version__)
        store['ncases'] = np.array(len(CASES))
        store['rv'] = np.array(RVS)
        store['radii'] = np.array(RADII)
        for c, (r_inst, r_samp) in enumerate(CASES):
            if r_samp is not None:
                f = 0.5 / r_samp
                g = (1.0 + f) / (1.0 - f)
                wn_min = 4000.0
                wn = ps.constant_resolution_spectrum(wn_min, wn_min * g**(NWAVE - 0.5), r_samp)
            else:
                wn = 6000.0 + 0.05 * np.arange(NWAVE)
            nwave = len(wn)
            assert nwave <= 16000
            x = np.linspace(0.0, 1.0, nwave)
            # a transit-depth-like spectrum (positive, lines on a slope) and an eclipse case
            lines = np.zeros(nwave)
            for pos, width, amp in zip(rng.uniform(0, 1, 60), rng.uniform(2e-4, 5e-3, 60),
                                       rng.uniform(1e-4, 2e-3, 60)):
                lines += amp * np.exp(-0.5 * ((x - pos) / width)**2)
            depth = f32(0.0101 + 5e-4 * x + lines + 2e-5 * rng.standard_normal(nwave))
            fplanet = f32(3.0e4 * (1.0 + 0.4 * np.sin(37.0 * x) + 0.3 * rng.uniform(size=nwave)))
            starflux = f32(2.1e6 * (1.0 + 0.1 * np.cos(11.0 * x) - 0.2 * lines / lines.max()))
            assert depth.min() > 0 and fplanet.min() > 0 and starflux.min() > 0
            # pyrat/spectrum.py:401-404
            fstar_rprs = 1 / starflux * (RADII[0] / RADII[1])**2
            eclipse = fplanet * fstar_rprs

            conv = {}
            for name, spectrum in (('depth', depth), ('eclipse', eclipse)):
                conv[name] = ps.inst_convolution(wn, spectrum, r_inst, sampling_res=r_samp)
            taps = taps_seen[-1]
            assert np.array_equal(taps_seen[-2], taps) and len(taps) % 2 == 1
            half = (len(taps) - 1) // 2
            assert 2 * half + 1 < nwave // 4

            tag = f'c{c}'
            store[f'{tag}_resolution'] = np.array([r_inst, np.nan if r_samp is None else r_samp])
            store[f'{tag}_wn'] = wn
            store[f'{tag}_taps'] = taps
            store[f'{tag}_depth'] = depth
            store[f'{tag}_fplanet'] = fplanet
            store[f'{tag}_starflux'] = starflux
            store[f'{tag}_depth_convolved'] = conv['depth']
            store[f'{tag}_eclipse_convolved'] = conv['eclipse']
            for r, rv in enumerate(RVS):
                shifted = ps.rv_shift(rv, wn=wn)
                # on shifted nodes (both ends of the grid among them), within (T - 1) / 2 samples
                # of each end (the zero padding of mode='same'), the rest anywhere; shuffled
                nodes = np.concatenate([[0, 1, nwave - 2, nwave - 1],
                                        rng.choice(np.arange(2, nwave - 2), 12, replace=False)])
                near = max(half, 2)
                low = rng.uniform(shifted[0], shifted[near], 12)
                high = rng.uniform(shifted[nwave - 1 - near], shifted[-1], 12)
                rest = rng.uniform(shifted[0], shifted[-1], NDATA - len(nodes) - 24)
                data_wn = np.concatenate([shifted[nodes], low, high, rest])
                rng.shuffle(data_wn)
                assert len(data_wn) == NDATA
                store[f'{tag}_rv{r}_data_wn'] = data_wn
                store[f'{tag}_rv{r}_on_node'] = np.array(np.sum(np.isin(data_wn, shifted)))
                for name in ('depth', 'eclipse'):
                    store[f'{tag}_rv{r}_{name}_sampled'] = si.interp1d(shifted, conv[name])(data_wn)
        out = os.path.join(HERE, 'g21_hires.npz')
        np.savez_compressed(out, **store)
        for k, v in store.items():
            if v.ndim and v.size > 4:
                print(k, v.shape, v.dtype)
        print(os.path.getsize(out), 'bytes')
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
