#!/usr/bin/env python3
"""The nested sampler's loop at the case of tools/bench_retrieval.py / bench_sampler.py: the C5
shape in emission geometry (80 layers x 1e5 samples, 24 bands, a free stellar temperature, offsets
and error scaling), 12 free parameters, seed 7, with nlive = 256 live points and a batch of 64.

Legs, each the median of `--blocks` timed blocks after a warm-up (min ... max beside it; wall clock
around a device synchronise), alternating block by block in one process:
  l  Retrieval.log_likelihood on a resident copy of the sampler's latest points (64 walkers),
     `--steps` calls per block
  b  one iteration of NestedSampler: pb_nested_select, then `--steps` walk steps of
     pb_nested_propose, prior_transform, log_likelihood, pb_nested_accept; nothing read back
  c  the same iteration driven from the host (nested.run_host over the device's prior_transform
     and log_likelihood: NumPy select and propose, upload, read-back, host accept)
and the launches alone, back to back between two device events: propose, prior_transform, accept,
select at nlive = 256 (batch 64) and at nlive = 4096 (batch 1024), finish and resample.  Prints one
JSON line.  Measured: profiles/nested.md.

    python tools/bench_nested.py [--steps K] [--blocks B] [--warmup W]
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

NLIVE, BATCH = 256, bench_c5.BATCH
SEED = 7


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import engine, nested
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
    nsteps = args.steps

    def sync():
        torch.cuda.synchronize()

    ns = ret.nested(nlive=NLIVE, seed=SEED, dlogz=None, batch=BATCH, nsteps=nsteps)

    def leg_b(i):
        ns.run(1)

    latest = [ns.live_u[:BATCH].clone()]

    def leg_l(i):
        return ret.log_likelihood(ret.prior_transform(latest[0]))

    # leg c: the same iterations driven from the host
    def log_like(theta):
        return ret.log_likelihood(engine.dev(theta)).cpu().numpy()

    def prior_transform(cube):
        return ret.prior_transform(engine.dev(cube)).cpu().numpy()
    host = [nested.run_host(log_like, prior_transform, NLIVE, BATCH, nsteps, 0, seed=SEED,
                            nfree=ret.nfree)]

    def leg_c(i):
        host[0] = nested.run_host(log_like, prior_transform, NLIVE, BATCH, nsteps, 1, seed=SEED,
                                  state=host[0])

    for i in range(args.warmup):
        leg_b(i), leg_c(i), leg_l(i)
    sync()
    res = {'workload': 'c5-emission-nested', 'nlive': NLIVE, 'batch': BATCH, 'nsteps': nsteps,
           'blocks': args.blocks, 'nfree': ret.nfree, 'nbands': nb}
    ll, lb, lc = [], [], []
    for _ in range(args.blocks):
        latest[0] = ns.point.clone()
        ll.append(block(leg_l, nsteps, sync))
        lb.append(block(leg_b, 1, sync))
        lc.append(block(leg_c, 1, sync))
    res['l_log_likelihood_per_step'] = summary(ll)
    res['b_iteration'] = summary(lb)
    res['c_host_iteration'] = summary(lc)
    res['b_per_step_ms'] = res['b_iteration']['median_ms'] / nsteps
    res['c_per_step_ms'] = res['c_host_iteration']['median_ms'] / nsteps
    res['per_block_ms'] = {'l': ll, 'b': lb, 'c': lc}
    res['iterations'] = int(ns.it)
    res['same_dead_b_c'] = bool(np.array_equal(ns.dead_idx.cpu().numpy(), host[0].dead_idx[-1]))
    res['efficiency'] = float(ns.efficiency())
    res['stuck'] = int(ns.stuck())
    res['logz'] = [float(v) for v in ns.logz().cpu().numpy()]

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

    def scratch_sampler(nlive, batch):
        """A started sampler on a cheap target, for the launches whose cost does not depend on
        the log-likelihood; its tensors are scratch: the launches below overwrite them."""
        s = nested.NestedSampler(lambda t: t.sum(dim=1), lambda c: c, ret.nfree, nlive,
                                 batch=batch, nsteps=nsteps, seed=SEED).start()
        return s.run(1)

    def launches(s):
        never = torch.full((s.K,), -float('inf'), dtype=torch.float64, device='cuda')

        def select():
            call('pb_nested_select', _ptr(s.dead_idx), _ptr(s.surv_idx), _ptr(s.dead_u),
                 _ptr(s.dead_logl), _ptr(s.dead_logw), _ptr(s.state), _ptr(s.live_u),
                 _ptr(s.live_logl), 0, s.dead_cap, s.K, s.nlive, s.nfree, _stream())

        def propose():
            call('pb_nested_propose', _ptr(s.point), _ptr(s.inside), _ptr(s.draw_a),
                 _ptr(s.draw_b), _ptr(s.draw_gamma), _ptr(s.cur), _ptr(s.cur_logl),
                 _ptr(s.acc_it), _ptr(s.live_u), _ptr(s.live_logl), _ptr(s.surv_idx), 1, 1,
                 s.seed, s.fgamma, s.p_unit, 1, s.nlive, s.nfree, s.K, _stream())

        def accept():
            # (a reject everywhere: the state is left as it is however often the launch runs)
            call('pb_nested_accept', _ptr(s.cur), _ptr(s.cur_logl), _ptr(s.point), _ptr(never),
                 _ptr(s.inside), _ptr(s.state), _ptr(s.naccept), _ptr(s.acc_it),
                 _ptr(s.stuck_slots), _ptr(s.accepted), _ptr(s.live_u), _ptr(s.live_logl),
                 _ptr(s.dead_idx), 0, s.nlive, s.nfree, s.K, _stream())
        return select, propose, accept

    small, large = scratch_sampler(NLIVE, BATCH), scratch_sampler(4096, 1024)
    select, propose, accept = launches(small)
    select_large, _, _ = launches(large)
    res['launches_ms'] = {
        'pb_nested_propose': timed(propose), 'pb_nested_accept': timed(accept),
        'prior_transform': timed(lambda: ret.prior_transform(latest[0])),
        'pb_nested_select_256_64': timed(select),
        'pb_nested_select_4096_1024': timed(select_large),
        'pb_nested_finish': timed(lambda: ns.logz(), 50),
        'finish_and_resample': timed(lambda: ns.unique(), 50),
        'note': 'back-to-back launches between two events, host submission included'}
    k = res['launches_ms']
    res['new_launches_per_step_ms'] = k['pb_nested_propose'] + k['pb_nested_accept'] + \
        k['pb_nested_select_256_64'] / nsteps
    res['new_launches_share_of_log_likelihood'] = res['new_launches_per_step_ms'] / \
        res['l_log_likelihood_per_step']['median_ms']
    res['select_4096_share_of_log_likelihood'] = k['pb_nested_select_4096_1024'] / \
        res['l_log_likelihood_per_step']['median_ms']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
