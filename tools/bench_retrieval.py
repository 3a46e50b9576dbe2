#!/usr/bin/env python3
"""The C5 retrieval batch in emission geometry from what a sampler holds, theta[64, nfree], to the
walkers' LOG-POSTERIORS: the model of tools/bench_loglike.py (64 walkers x 80 layers x 1e5 samples,
an eclipse with a free stellar temperature, 24 bands over three instruments, 3 offset and 2 error
models) behind a 14-line retrieval_params block with a fixed and a shared line (12 free
parameters; the offset and the error model no line names are constants of the map), seed 7.

Three legs, each the median of `--blocks` timed blocks of `--steps` batches after a warm-up
(min ... max beside it; wall clock around a device synchronise), alternating block by block in
one process on the same walkers:
  a  eval_loglike on hand-split tensors that are already resident (the launches the loop had)
  b  Retrieval.log_posterior(theta): pb_retrieval_map, the same launches, pb_log_posterior
  c  what a caller did before: torch slicing and scaling of theta into the same tensors, a NumPy
     prior on the host copy of theta, eval_loglike, and the sum
and the three new launches alone, back to back between two device events.  Prints one JSON line.
Measured: profiles/retrieval.md.

    python tools/bench_retrieval.py [--steps K] [--blocks B] [--warmup W]
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

BATCH = bench_c5.BATCH
#   name          value    pmin     pmax   pstep    prior priorlow priorup
BLOCK = """
    log_kappa'     -1.5    -4.0      1.0    0.1
    log_gamma1     -0.8    -3.0      1.0    0.1
    log_gamma2     -0.8    -3.0      1.0   -2
    alpha           0.5
    T_irr        1200.0   300.0   2500.0   30.0   1250.0   100.0   200.0
    T_int         100.0     0.0    500.0   10.0
    log_H2O        -3.4    -9.0     -1.0    0.1
    log_CO         -3.3    -9.0     -1.0    0.1
    log_CH4        -4.0    -9.0     -1.0    0.1
    R_planet        1.0     0.5      2.0    0.02     1.0     0.05
    T_eff        5400.0  4000.0   6750.0  100.0   5400.0   150.0
    offset_nrs1     0.0   {omin}   {omax}   {ostep}
    offset_miri     0.0   {omin}   {omax}   {ostep}
    err_scale_nrs1  0.0    -1.0      1.0    0.1
"""


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import engine
    from pyratbay_amd.retrieval import RUNITS
    torch.cuda.set_device(0)
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
    rng = np.random.default_rng(7)
    base = np.array(bench_c5_atmosphere.BASE)
    first = model.eval_params(watm, engine.dev(base[None, :]), pb,
                              tstar=engine.dev(np.full(1, 5400.0)), chunk=bench_c5.CHUNK)
    level = first.cpu().numpy()[0]
    assert np.all(np.isfinite(level))
    names = [INSTRUMENTS[(3 * b) // nb] for b in range(nb)]
    obs = engine.Observation(level * (1 + rng.normal(0, 0.02, nb)), 0.03 * level, names, OFFSETS,
                             ERRORS, units='ppm')
    scale = float(np.max(level)) * 1e6
    text = BLOCK.format(omin=-0.05 * scale, omax=0.05 * scale, ostep=0.005 * scale)
    ret = engine.Retrieval(model, watm, pb, obs, text, chunk=bench_c5.CHUNK)
    f = ret.ifree
    theta_h = [ret.params[f] + ret.pstep[f] * rng.uniform(-1, 1, (BATCH, ret.nfree))
               for _ in range(4)]
    assert all(np.all(ret.inside_host(t)) for t in theta_h)
    theta = [engine.dev(t) for t in theta_h]
    # leg a: the tensors of the map, made beforehand
    split = [{k: engine.dev(v) for k, v in ret.split_host(t).items()} for t in theta_h]

    def sync():
        torch.cuda.synchronize()

    def leg_a(i):
        s = split[i % 4]
        return model.eval_loglike(watm, s['params'], pb, obs, offsets=s['offsets'],
                                  err_pars=s['err_pars'], tstar=s['tstar'], chunk=bench_c5.CHUNK)

    def leg_b(i):
        return ret.log_posterior(theta[i % 4])

    # leg c: the caller's own slicing, by the names and positions it has to know
    free_names = [ret.pnames[i] for i in f]
    col = {n: free_names.index(n) for n in free_names}
    atm_cols = [col[n] for n in ("log_kappa'", 'log_gamma1', 'log_gamma1')]
    tail_cols = [col[n] for n in ('T_irr', 'T_int', 'log_H2O', 'log_CO', 'log_CH4')]
    rjup = RUNITS['rjup']
    quad_default = float(obs.err_defaults[1])

    def leg_c(i):
        k = i % 4
        t = theta[k]
        nw = t.shape[0]
        params = torch.empty((nw, watm.npar), dtype=torch.float64, device='cuda')
        params[:, 0:3] = t[:, atm_cols]
        params[:, 3] = 0.5
        params[:, 4:9] = t[:, tail_cols]
        params[:, 9] = t[:, col['R_planet']] * rjup
        offsets = torch.zeros((nw, 3), dtype=torch.float64, device='cuda')
        offsets[:, 0] = t[:, col['offset_nrs1']]
        offsets[:, 2] = t[:, col['offset_miri']]
        err_pars = torch.full((nw, 2), quad_default, dtype=torch.float64, device='cuda')
        err_pars[:, 0] = t[:, col['err_scale_nrs1']]
        tstar = t[:, col['T_eff']].contiguous()
        prior = ret.log_prior_host(theta_h[k])
        ll = model.eval_loglike(watm, params, pb, obs, offsets=offsets, err_pars=err_pars,
                                tstar=tstar, chunk=bench_c5.CHUNK)
        return ll + engine.dev(prior)

    for i in range(args.warmup):
        leg_a(i), leg_b(i), leg_c(i)
    sync()
    a0, b0, c0 = (leg(0).cpu().numpy() for leg in (leg_a, leg_b, leg_c))
    live = a0 > -1e90
    res = {'workload': 'c5-emission-retrieval', 'walkers_per_batch': BATCH, 'steps': args.steps,
           'blocks': args.blocks, 'lines': ret.npar, 'nfree': ret.nfree, 'mapped': ret.nmap,
           'destinations': ret.dest_names, 'nbands': nb,
           'rejected_walkers': int((~live).sum()),
           'b_equals_a_plus_prior': bool(np.array_equal(b0, a0 + ret.log_prior_host(theta_h[0]))),
           'c_equals_b': bool(np.array_equal(c0, b0))}
    la, lb, lc = [], [], []
    for _ in range(args.blocks):
        la.append(block(leg_a, args.steps, sync))
        lb.append(block(leg_b, args.steps, sync))
        lc.append(block(leg_c, args.steps, sync))
    res['a_eval_loglike'] = summary(la)
    res['b_log_posterior'] = summary(lb)
    res['c_torch_route'] = summary(lc)
    res['b_minus_a_ms'] = res['b_log_posterior']['median_ms'] - res['a_eval_loglike']['median_ms']
    res['c_minus_a_ms'] = res['c_torch_route']['median_ms'] - res['a_eval_loglike']['median_ms']
    res['a_spread_ms'] = res['a_eval_loglike']['max_ms'] - res['a_eval_loglike']['min_ms']

    def timed(fn, reps=200):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(10):
            fn()
        ev0.record()
        for _ in range(reps):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / reps

    args0 = ret.arguments(theta[0])
    ll = leg_a(0)
    cube = engine.dev(rng.uniform(0.01, 0.99, (BATCH, ret.nfree)))
    res['kernels_ms'] = {
        'pb_retrieval_map': timed(lambda: ret.arguments(theta[0])),
        'pb_log_posterior': timed(lambda: ret._combine(ll, args0, -np.inf, True)),
        'pb_prior_transform': timed(lambda: ret.prior_transform(cube)),
        'note': 'back-to-back launches between two events, host submission and the output '
                'allocations of the wrappers included'}
    res['two_launches_ms'] = res['kernels_ms']['pb_retrieval_map'] + \
        res['kernels_ms']['pb_log_posterior']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
