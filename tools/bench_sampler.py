#!/usr/bin/env python3
"""One generation of the sampler at the case of tools/bench_retrieval.py: 64 chains at the C5
shape in emission geometry (80 layers x 1e5 samples, 24 bands, a free stellar temperature,
offsets and error scaling), 12 free parameters, seed 7.

Three legs, each the median of `--blocks` timed blocks of `--steps` generations after a warm-up
(min ... max beside it; wall clock around a device synchronise), alternating block by block in
one process:
  a  Retrieval.log_posterior on a resident theta, the starting states (what a generation cannot
     do without)
  a' the same on a resident copy of the sampler's latest proposals, taken anew before every
     block: the cost of log_posterior depends on where the walkers are
  b  one DEMC generation: pb_demc_propose, log_posterior, pb_demc_accept, nothing read back
  c  the loop a caller had to write: NumPy proposal (sampler.propose_host), upload,
     log_posterior, read-back, host accept (sampler.accept_host)
and the two new launches alone, back to back between two device events.  Prints one JSON line.
Measured: profiles/sampler.md.

    python tools/bench_sampler.py [--steps K] [--blocks B] [--warmup W]
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

BATCH = bench_c5.BATCH
SEED = 7


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import engine, sampler
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
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
    rng = np.random.default_rng(SEED)
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
    pstep = ret.pstep[f]
    z0 = ret.params[f] + pstep * rng.uniform(-1, 1, (10 * BATCH, ret.nfree))
    assert np.all(ret.inside_host(z0))
    ngen = (args.warmup + args.blocks * args.steps) + 16
    kw = dict(fepsilon=0.01, thin_z=10)

    def sync():
        torch.cuda.synchronize()

    theta = engine.dev(z0[-BATCH:])

    def leg_a(i):
        return ret.log_posterior(theta)

    demc = engine.DEMC(ret.log_posterior, ret.nfree, pstep, seed=SEED, **kw)
    demc.start(z0[-BATCH:], z0, ngen + 1)

    def leg_b(i):
        demc.run(1)

    latest = [demc.prop]

    def leg_a2(i):
        return ret.log_posterior(latest[0])

    # leg c: the same generation driven from the host
    start = z0[-BATCH:].copy()
    st = sampler.new_state_host(start, ret.log_posterior(engine.dev(start)).cpu().numpy(), z0,
                                ngen + 1, thin_z=kw['thin_z'])

    def leg_c(i):
        gen = st.g + 1
        prop, log_jac, _ = sampler.propose_host(st.theta, st.z, st.M, pstep, gen, SEED,
                                                fepsilon=kw['fepsilon'])
        logp_prop = ret.log_posterior(engine.dev(prop)).cpu().numpy()
        append = gen % kw['thin_z'] == 0 and st.M + BATCH <= st.Mcap
        sampler.accept_host(st, prop, logp_prop, log_jac, gen, SEED, append)
        st.M += BATCH if append else 0
        st.g = gen

    for i in range(args.warmup):
        leg_a(i), leg_b(i), leg_c(i)
    sync()
    res = {'workload': 'c5-emission-sampler', 'chains': BATCH, 'steps': args.steps,
           'blocks': args.blocks, 'nfree': ret.nfree, 'nbands': nb, 'history_rows': int(demc.M),
           'same_decisions_b_c': bool(np.array_equal(demc.nrows.cpu().numpy(), st.nrows))}
    la, la2, lb, lc = [], [], [], []
    for _ in range(args.blocks):
        la.append(block(leg_a, args.steps, sync))
        latest[0] = demc.prop.clone()
        la2.append(block(leg_a2, args.steps, sync))
        lb.append(block(leg_b, args.steps, sync))
        lc.append(block(leg_c, args.steps, sync))
    res['a_log_posterior'] = summary(la)
    res['a2_log_posterior_of_proposals'] = summary(la2)
    res['b_demc_generation'] = summary(lb)
    res['c_host_loop'] = summary(lc)
    res['b_minus_a_ms'] = res['b_demc_generation']['median_ms'] - \
        res['a_log_posterior']['median_ms']
    res['b_minus_a2_ms'] = res['b_demc_generation']['median_ms'] - \
        res['a2_log_posterior_of_proposals']['median_ms']
    res['per_block_ms'] = {'a': la, 'a2': la2, 'b': lb, 'c': lc}
    res['c_minus_a_ms'] = res['c_host_loop']['median_ms'] - res['a_log_posterior']['median_ms']
    res['a_spread_ms'] = res['a_log_posterior']['max_ms'] - res['a_log_posterior']['min_ms']
    res['generations'] = int(demc.g)
    res['same_decisions_b_c_after'] = bool(np.array_equal(demc.nrows.cpu().numpy(), st.nrows))
    res['acceptance'] = float(demc.acceptance().mean())

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

    d = demc
    # (a reject everywhere: the store is left as it is however often the launch runs)
    never = torch.full((BATCH,), -float('inf'), dtype=torch.float64, device='cuda')
    stat = {k: getattr(d, k).clone() for k in ('mean', 'm2', 'nstat', 'counts')}

    def propose():
        call('pb_demc_propose', _ptr(d.prop), _ptr(d.log_jac), _ptr(d.kind), _ptr(d.theta),
             _ptr(d.z), _ptr(d.pstep), d.g + 1, d.seed, d.M, d.fgamma, d.fepsilon, d.p_snooker,
             d.nfree, d.nw, _stream())

    def accept():
        call('pb_demc_accept', _ptr(d.theta), _ptr(d.logp), _ptr(d.prop), _ptr(never),
             _ptr(d.log_jac), _ptr(d.rows), _ptr(d.row_logp), _ptr(d.row_gen), _ptr(stat['counts']),
             _ptr(d.nrows), _ptr(d.overflow), _ptr(stat['mean']), _ptr(stat['m2']),
             _ptr(stat['nstat']), _ptr(d.z), _ptr(d.accepted), d.g + 1, d.seed, d.M, d.Mcap, 0,
             d.cap, d.nfree, d.nw, _stream())

    res['kernels_ms'] = {
        'pb_demc_propose': timed(propose), 'pb_demc_accept': timed(accept),
        'note': 'back-to-back launches between two events, host submission included'}
    res['two_launches_ms'] = res['kernels_ms']['pb_demc_propose'] + \
        res['kernels_ms']['pb_demc_accept']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
