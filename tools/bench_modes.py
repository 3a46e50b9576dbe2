#!/usr/bin/env python3
"""The mode decomposition of a nested-sampling run (pyratbay_amd/modes.py, csrc/pb_modes.hip) at
N = 1e5 stored points and 4096 rows, for 16 and 128 free parameters: a dead store filled by hand
with two blobs in the unit cube (no model behind it), 4096 live points.

Per shape, each figure the median of `--blocks` timed blocks of `--reps` calls after `--warmup`
blocks (min ... max beside it; device events around the block):
  modes        NestedSampler.modes(): finish, resample, rows, link, assign, evidence, two counts
               read back
  link         pb_modes_link alone (nearest rows, ell2, the bit matrix, the components)
  assign       pb_modes_assign alone, with its 3 N n nfree flops per second and their share of the
               FP64 vector rate: 78.6 TFLOP/s, half the FP32 vector rate of MI355X_MICROARCH.md
               (AMD's data sheet; a rate that counts a fused multiply-add as two, and the kernel
               fuses nothing because the statement rounds every operation)
  evidence     pb_modes_evidence alone, two modes
  cdist        torch.cdist + argmin over the labelled rows on the device: for time only, its bits
               are not the statement's
  host         modes.assign_host (NumPy) at `--host-points` points, scaled to N
Prints one JSON line; sets no pass mark.  Measured: profiles/modes.md.

    python tools/bench_modes.py [--points N] [--reps R] [--blocks B] [--warmup W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NLIVE = 4096
FP64_VECTOR_FLOPS = 78.6e12


def fake_run(engine, nfree, npoints, seed):
    """A started sampler whose dead store is filled by hand: two blobs of 2/3 and 1/3 of the
    points, ln X falling by 1 / nlive per death."""
    import torch
    rng = np.random.default_rng(seed)
    ns = engine.NestedSampler(lambda t: -0.5 * torch.sum((t - 0.5)**2, dim=1), lambda c: c, nfree,
                              NLIVE, batch=NLIVE // 4, nsteps=1, seed=seed).start()
    ndead = (npoints - NLIVE) // ns.K * ns.K

    def blobs(n):
        centre = np.where(rng.uniform(0, 1, (n, 1)) < 2.0 / 3.0, 0.3, 0.7)
        return centre + rng.normal(0.0, 0.02, (n, nfree))
    ns._grow(ndead)
    # (logl rises as fast as ln X falls: equal weights, so that the 4096 draws fall on about as
    # many rows)
    logl = np.arange(ndead) / float(NLIVE)
    logw = logl - np.arange(ndead) / float(NLIVE) + np.log(-np.expm1(-1.0 / NLIVE))
    ns.dead_u[:ndead] = engine.dev(blobs(ndead))
    ns.dead_logl[:ndead] = engine.dev(logl)
    ns.dead_logw[:ndead] = engine.dev(logw)
    ns.live_u.copy_(engine.dev(blobs(NLIVE)))
    ns.live_logl.copy_(engine.dev(logl[-1] + rng.exponential(0.1, NLIVE)))
    ns.state[0] = -ndead / float(NLIVE)
    ns.it = ndead // ns.K
    return ns


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--points', type=int, default=100000)
    ap.add_argument('--host-points', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import engine, modes
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
    engine.require_gpu()
    torch.cuda.set_device(0)

    def timed(fn):
        """ms per call: median, min, max over the blocks."""
        out = []
        for b in range(args.warmup + args.blocks):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.reps):
                fn()
            end.record()
            end.synchronize()
            if b >= args.warmup:
                out.append(start.elapsed_time(end) / args.reps)
        return dict(median_ms=float(np.median(out)), min_ms=min(out), max_ms=max(out))

    res = dict(points=args.points, reps=args.reps, blocks=args.blocks, warmup=args.warmup,
               fp64_vector_flops=FP64_VECTOR_FLOPS, shapes={})
    for nfree in (16, 128):
        ns = fake_run(engine, nfree, args.points, 7 + nfree)
        md = ns.modes()
        cube = ns._cube().contiguous()
        N, n = cube.shape[0], md.rows.shape[0]
        R = cube[md.rows].contiguous()
        out, logw, logl, _ = ns._finish()
        labels = torch.empty_like(md.labels)
        count = torch.empty(1, dtype=torch.int32, device='cuda')
        ell2, dk = torch.empty(1, dtype=torch.float64, device='cuda'), torch.empty_like(R[:, 0])
        bits = torch.empty(n * ((n + 31) // 32), dtype=torch.int32, device='cuda')
        mode = torch.empty_like(md.mode)
        triple = [torch.empty(md.nmodes, dtype=torch.float64, device='cuda') for _ in range(3)]
        has = md.labels >= 0

        def link():
            call('pb_modes_link', _ptr(labels), _ptr(count), _ptr(ell2), _ptr(dk), _ptr(bits),
                 _ptr(R), n, nfree, 10, 1.0, modes.default_min_mode(nfree), 16, _stream())

        def assign():
            call('pb_modes_assign', _ptr(mode), _ptr(cube), _ptr(R), _ptr(md.labels), N, n, nfree,
                 _stream())

        def evidence():
            call('pb_modes_evidence', *(_ptr(t) for t in triple), _ptr(logw), _ptr(logl),
                 _ptr(md.mode), _ptr(out), N, md.nmodes, _stream())

        def cdist():
            return md.labels[has][torch.argmin(torch.cdist(cube, R[has]), dim=1)]
        shape = dict(N=N, rows=n, nmodes=md.nmodes, modes=timed(ns.modes), link=timed(link),
                     assign=timed(assign), evidence=timed(evidence), cdist=timed(cdist))
        assert torch.equal(mode, md.mode) and torch.equal(labels, md.labels)
        shape['cdist_labels_that_differ'] = int((cdist() != md.mode).sum())
        flops = 3.0 * N * n * nfree
        shape['assign']['flops'] = flops
        shape['assign']['tflops'] = flops / (shape['assign']['median_ms'] * 1e-3) / 1e12
        shape['assign']['share_of_fp64_vector_rate'] = shape['assign']['tflops'] * 1e12 / \
            FP64_VECTOR_FLOPS
        P, Rh, lh = cube[:args.host_points].cpu().numpy(), R.cpu().numpy(), md.labels.cpu().numpy()
        t0 = time.perf_counter()
        want = modes.assign_host(P, Rh, lh)
        host_s = time.perf_counter() - t0
        assert np.array_equal(want, md.mode[:args.host_points].cpu().numpy())
        shape['host'] = dict(points=args.host_points, measured_ms=host_s * 1e3,
                             scaled_to_N_ms=host_s * 1e3 * N / args.host_points)
        res['shapes'][f'nfree_{nfree}'] = shape
    print(json.dumps(res))


if __name__ == '__main__':
    main()
