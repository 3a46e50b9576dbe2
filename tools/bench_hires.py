#!/usr/bin/env python3
"""High-resolution data in the retrieval batch at C5's shape (1e5 wavenumbers x 80 layers, 64
walkers): ms per 64 walkers of
  (a) eval_bands with PassBands (the existing exit, for comparison),
  (b) eval_bands with HiresData at ndata = 2 000, 20 000 and W, R_inst = 5 000 and 25 000,
  (c) the observation step alone, fused (one launch, no [nw, W] intermediate),
  (d) the same step as convolve() + a separate sampling launch,
  (e) the same step on the CPU with the SciPy calls the reference makes (one walker timed, x 64).
One JSON line per measurement; `--out FILE` also writes them to a file.

    python tools/bench_hires.py [--steps 20] [--warmup 3] [--no-cpu] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def cpu_step(wn, spectrum, resolution, data_wn, rv):
    """inst_convolution's SciPy calls + rv_shift + interp1d for one walker (seconds)."""
    import scipy.interpolate as si
    from scipy.signal import convolve
    from pyratbay_amd import hires
    t0 = time.perf_counter()
    taps = hires.inst_kernel(resolution, wn=wn)
    conv = convolve(spectrum, taps, mode='same')
    si.interp1d(wn * hires.doppler_factor(rv), conv)(data_wn)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--small', action='store_true', help='a 1e4-wavenumber model (a quick look)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from pyratbay_amd import engine as eng, hires
    from tools import bench_c5
    from tools.gpu_state import Sampler
    eng.require_gpu()
    nwalk = 64
    inp = bench_c5.inputs(nwave=10001, nlayers=40) if args.small else bench_c5.inputs()
    g, atm = inp['grid'], inp['atm']
    wn, nwave = g['wn'], g['nwave']
    temps, dens, radius = bench_c5.walkers(inp, nwalk, 700)
    td, dd, rd = eng.dev(temps), eng.dev(dens), eng.dev(radius)
    rng = np.random.default_rng(1)
    rv_max = 30.0
    rv = rng.uniform(-rv_max, rv_max, nwalk)
    rvd = eng.dev(rv)
    model = eng.TableSpectrum(inp['etable'], inp['ttable'], wn, atm['radius'], atm['rstar'])
    bands = eng.PassBands(wn, inp['bands'])
    rows = []
    state = Sampler()

    def record(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    with state:
        ms = timed(lambda: model.eval_bands(td, dd, bands, radius=rd, chunk=nwalk), args.steps,
                   args.warmup)
        record(what='a eval_bands PassBands', nwave=nwave, ms_per_64=round(ms, 4))

        class Capture:
            nbands = 1

            def integrate_batch(self, s, out=None, f_dilution=None):
                self.spectra = s.clone()
                return out.zero_()
        cap = Capture()
        model.eval_bands(td, dd, cap, radius=rd, chunk=nwalk)
        spectra = cap.spectra
        lo, hi = wn[0] * hires.doppler_factor(-rv_max), wn[-1] * hires.doppler_factor(rv_max)
        for resolution in (5000.0, 25000.0):
            for ndata in (2000, 20000, nwave):
                data_wn = rng.uniform(lo, hi, ndata)
                h = eng.HiresData(wn, data_wn, resolution, rv_max=rv_max)
                out = torch.empty((nwalk, ndata), dtype=torch.float64, device='cuda')
                common = dict(R_inst=resolution, ndata=ndata, ntaps=len(h.taps_host), nwave=nwave)
                ms = timed(lambda: model.eval_bands(td, dd, h, radius=rd, chunk=nwalk, rv=rvd),
                           args.steps, args.warmup)
                record(what='b eval_bands HiresData', ms_per_64=round(ms, 4), **common)
                h.fused = True
                ms_c = timed(lambda: h.integrate_batch(spectra, out=out, rv=rvd), args.steps,
                             args.warmup)
                record(what='c observe fused', ms_per_64=round(ms_c, 4),
                       spectra_read_TBps=round(spectra.numel() * 8 / ms_c / 1e9, 3), **common)
                h.fused = False
                ms_d = timed(lambda: h.integrate_batch(spectra, out=out, rv=rvd), args.steps,
                             args.warmup)
                record(what='d convolve + sample', ms_per_64=round(ms_d, 4), **common)
                if not args.no_cpu:
                    try:
                        sec = min(cpu_step(wn, spectra[0].cpu().numpy(), resolution, data_wn,
                                           rv[0]) for _ in range(3))
                        record(what='e SciPy on the CPU', s_per_64=round(64 * sec, 4), **common)
                    except ImportError:
                        record(what='e SciPy on the CPU', s_per_64=None, note='no SciPy', **common)
    record(what='gpu_state', gpu_state=state.summary())
    if args.out:
        with open(args.out, 'w') as f:
            for row in rows:
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
