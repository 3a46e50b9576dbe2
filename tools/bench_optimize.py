#!/usr/bin/env python3
"""The batched Levenberg-Marquardt iteration at the case of tools/bench_loglike.py /
bench_nested.py: the C5 shape in emission geometry (80 layers x 1e5 samples, 24 bands, a free
stellar temperature, offsets), the block of bench_retrieval.py with its error-scaling line fixed
(a free one is refused), 64 starts, seed 7.

Legs, each the median of `--blocks` timed blocks after a warm-up (min ... max beside it; wall clock
around a device synchronise), alternating block by block in one process:
  e  the two residual calls an iteration contains, alone: Retrieval.residuals on resident copies
     of the probe points (64 (nfree + 1) walkers) and of the trial points (64 x 4): the floor
  b  one iteration of LevenbergMarquardt: pb_lm_probe, residuals, pb_lm_normal, pb_lm_step,
     residuals, pb_lm_update; nothing read back
  c  the same iteration driven from the host (optimize.lm_host over Retrieval.residuals: NumPy
     probe, normal equations, Cholesky and update, an upload and a read-back per residual call)
and pb_lm_normal alone, back to back between two device events, on synthetic residuals of
m = 1e3, 1e4 and 1e5 columns for 64 starts at the case's nfree and at nfree = 128, with its
traffic (one read of R) and its FP64 multiply-add count.  Prints one JSON line.  Measured:
profiles/optimize.md.

    python tools/bench_optimize.py [--blocks B] [--warmup W]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import bench_c5, bench_c5_atmosphere  # noqa: E402
from tools.bench_loglike import ERRORS, INSTRUMENTS, OFFSETS, block, stellar_grid, summary  # noqa: E402
from tools.bench_retrieval import BLOCK  # noqa: E402

NSTARTS, SEED = 64, 7
FREE_ERROR_LINE = 'err_scale_nrs1  0.0    -1.0      1.0    0.1'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--normal-only', action='store_true', help='pb_lm_normal alone')
    args = ap.parse_args()
    import torch
    from pyratbay_amd import engine, optimize
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
    torch.cuda.set_device(0)
    res = {'workload': 'c5-emission-optimize', 'nstarts': NSTARTS, 'blocks': args.blocks}

    def sync():
        torch.cuda.synchronize()

    nfree_case = 11
    if not args.normal_only:
        inp = bench_c5.inputs()
        g, atm = inp['grid'], inp['atm']
        wn, bands = g['wn'], inp['bands']
        nb = len(bands)
        watm = bench_c5_atmosphere.atmosphere(inp)
        rstar = float(atm['rstar'])
        model = engine.TableSpectrum(inp['etable'], inp['ttable'], wn, watm.base_radius, rstar,
                                     rt_path='emission')
        sed_temps, fluxes = stellar_grid(wn)
        grid = engine.StellarGrid(wn, sed_temps, fluxes)
        pb = engine.PassBands(wn, bands).set_eclipse_grid(rstar, grid)
        rng = np.random.default_rng(SEED)
        base = np.array(bench_c5_atmosphere.BASE)
        first = model.eval_params(watm, engine.dev(base[None, :]), pb,
                                  tstar=engine.dev(np.full(1, 5400.0)), chunk=bench_c5.CHUNK)
        level = first.cpu().numpy()[0]
        assert np.all(np.isfinite(level))
        names = [INSTRUMENTS[(3 * b) // nb] for b in range(nb)]
        obs = engine.Observation(level * (1 + rng.normal(0, 0.02, nb)), 0.03 * level, names,
                                 OFFSETS, ERRORS, units='ppm')
        scale = float(np.max(level)) * 1e6
        assert FREE_ERROR_LINE in BLOCK
        text = BLOCK.replace(FREE_ERROR_LINE, FREE_ERROR_LINE[:-3] + '0.0').format(
            omin=-0.05 * scale, omax=0.05 * scale, ostep=0.005 * scale)
        ret = engine.Retrieval(model, watm, pb, obs, text, chunk=bench_c5.CHUNK)
        f = ret.ifree
        nfree_case = ret.nfree
        theta0 = ret.params[f] + ret.pstep[f] * rng.uniform(-1, 1, (NSTARTS, ret.nfree))
        assert np.all(ret.inside_host(theta0))
        lm = engine.LevenbergMarquardt(ret.residuals, ret.nfree, ret.pmin[f], ret.pmax[f],
                                       ret.pstep[f], max_iter=10**6).start(theta0)
        lm.run(1)
        probe, trial = lm.probe.clone().view(-1, ret.nfree), lm.trial.clone().view(-1, ret.nfree)

        def leg_e(i):
            ret.residuals(probe), ret.residuals(trial)

        def leg_b(i):
            lm.run(1)

        def residuals_host(theta):
            return ret.residuals(engine.dev(theta)).cpu().numpy()
        kw = dict(max_iter=10**6)
        host = [optimize.lm_host(residuals_host, theta0, ret.pmin[f], ret.pmax[f], ret.pstep[f],
                                 niter=1, **kw)]

        def leg_c(i):
            host[0] = optimize.lm_host(residuals_host, theta0, ret.pmin[f], ret.pmax[f],
                                       ret.pstep[f], niter=1, state=host[0], **kw)

        for i in range(args.warmup):
            leg_e(i), leg_b(i), leg_c(i)
        sync()
        le, lb, lc = [], [], []
        for _ in range(args.blocks):
            le.append(block(leg_e, 1, sync))
            lb.append(block(leg_b, 1, sync))
            lc.append(block(leg_c, 1, sync))
        res.update(nfree=ret.nfree, nbands=nb, m=lm.m, ntrial=lm.s.ntrial,
                   walkers_per_iteration=NSTARTS * (ret.nfree + 1 + lm.s.ntrial),
                   e_two_residual_calls=summary(le), b_iteration=summary(lb),
                   c_host_iteration=summary(lc), per_block_ms={'e': le, 'b': lb, 'c': lc},
                   iterations=int(lm.done), unfinished=int(lm.unfinished.item()),
                   host_unfinished=int(host[0].unfinished),
                   best_cost=float(lm.cost.min().item()))
        res['b_over_e'] = res['b_iteration']['median_ms'] / res['e_two_residual_calls']['median_ms']
        res['c_over_b'] = res['c_host_iteration']['median_ms'] / res['b_iteration']['median_ms']

    def timed(fn, reps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            fn()
        ev0.record()
        for _ in range(reps):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / reps

    normal = {}
    for nfree in sorted({nfree_case, 128}):
        for m in (1000, 10000, 100000):
            gen = torch.Generator(device='cuda').manual_seed(SEED)
            R = torch.randn((NSTARTS, nfree + 1, m), dtype=torch.float64, device='cuda',
                            generator=gen)
            step = torch.full((NSTARTS, nfree), 1e-4, dtype=torch.float64, device='cuda')
            A = torch.empty((NSTARTS, nfree, nfree), dtype=torch.float64, device='cuda')
            gv = torch.empty((NSTARTS, nfree), dtype=torch.float64, device='cuda')
            cost = torch.empty(NSTARTS, dtype=torch.float64, device='cuda')

            def launch():
                call('pb_lm_normal', _ptr(A), _ptr(gv), _ptr(cost), _ptr(R), _ptr(step), nfree,
                     m, NSTARTS, _stream())
            ms = timed(launch, 20 if m < 100000 else 5)
            gbytes = 8.0 * R.numel() / 1e9
            tiles = -(-nfree // 32)
            # the multiply-adds the kernel issues: whole 32 x 32 tiles of the upper triangle
            fma = NSTARTS * m * 1024.0 * tiles * (tiles + 1) / 2
            normal[f'nfree{nfree}_m{m}'] = {
                'ms': ms, 'read_once_GBps': gbytes / (ms * 1e-3),
                'useful_Gfma_per_s': NSTARTS * m * nfree * (nfree + 1) / 2 / (ms * 1e6),
                'issued_Gfma_per_s': fma / (ms * 1e6)}
            del R
    res['pb_lm_normal'] = normal
    res['pb_lm_normal_note'] = ('back-to-back launches between two events, host submission '
                                'included; separate multiply and add (no contraction)')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
