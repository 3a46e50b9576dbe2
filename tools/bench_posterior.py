#!/usr/bin/env python3
"""The reduction of a posterior's spectrum store to its five quantiles (pyratbay_amd/posterior.py,
csrc/pb_quantiles.hip) at the grid of `bench.py --workload c5` (100001 wavenumbers) for n = 4096
unique samples (the column held in LDS) and n = 32768 (every pass re-reads it), with random
counts 0 ... 5.  The store [nwave, n] is synthetic: a base spectrum per wavenumber times
1 + 0.01 x a normal deviate per sample -- columns whose values share their leading bytes, like
the spectra of a converged chain.  Only the reduction is timed, not the evaluation of the samples.

Legs per n, each in ms for the whole store:
  kernel       posterior.weighted_quantiles with the sum of the counts given (ranks on the host,
               three small uploads, one launch of pb_weighted_quantiles)
  torch_route  the same result from torch alone, written here: torch.sort along n, cumsum of the
               gathered counts, searchsorted, gather, NumPy's lerp in torch ops -- in blocks of
               `--block` columns (the sort's temporaries of the whole store would not fit beside it)
  host_route   the reference's own route (tools/retrieval_tools.py:486-503): the store copied to
               the host, models[uinv], np.percentile per wavenumber -- measured on the first
               `--host-columns` columns and scaled to the grid (stated in the output)
and: whether torch_route and host_route have the kernel's bits, the kernel's fraction of the
one-read traffic bound (8 nwave n bytes at the copy rate `box_reference` measures on this card),
and the card's clocks while the kernel ran.  Prints one JSON line.

    python tools/bench_posterior.py [--samples 4096,32768] [--steps 5] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import bench_c5  # noqa: E402


def device_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def make_store(nwave, n, seed):
    """store[nwave, n] on the device, filled in blocks of columns."""
    import torch
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    base = 0.01 + 0.002 * torch.rand(nwave, dtype=torch.float64, device='cuda', generator=gen)
    store = torch.empty((nwave, n), dtype=torch.float64, device='cuda')
    for c0 in range(0, nwave, 4096):
        c1 = min(c0 + 4096, nwave)
        store[c0:c1] = torch.randn((c1 - c0, n), dtype=torch.float64, device='cuda',
                                   generator=gen)
        store[c0:c1].mul_(0.01).add_(1.0).mul_(base[c0:c1, None])
    return store


def torch_route(store, counts, rank_lo, rank_hi, gamma, block):
    import torch
    ncol, n = store.shape
    nq = gamma.shape[0]
    out = torch.empty((nq, ncol), dtype=torch.float64, device=store.device)
    ranks = torch.cat([rank_lo, rank_hi])
    t = gamma[None, :]
    for c0 in range(0, ncol, block):
        c1 = min(c0 + block, ncol)
        values, index = torch.sort(store[c0:c1], dim=1)
        ends = torch.cumsum(counts[index], dim=1)
        # the first row whose running count passes the rank (rows of count 0 never are)
        pos = torch.searchsorted(ends, ranks.expand(c1 - c0, -1).contiguous(), right=True)
        picked = values.gather(1, pos)
        a, b = picked[:, :nq], picked[:, nq:]
        d = b - a
        out[:, c0:c1] = torch.where(t >= 0.5, b - d * (1 - t), a + d * t).t()
    return out


def host_route(store, inverse, q100, columns):
    """-> (seconds for `columns` columns: copy + expansion + percentile, the quantiles)."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    models = store[:columns].t().cpu().numpy()              # [n, columns], as the reference has it
    out = np.empty((len(q100), columns))
    for i in range(columns):
        out[:, i] = np.percentile(models[inverse, i], q100)
    return time.perf_counter() - t0, out


def run(n, nwave, args, hbm_gbps):
    import torch
    from pyratbay_amd import _capi, engine, posterior
    from tools.gpu_state import Sampler
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 6, n)
    total = int(counts.sum())
    store = make_store(nwave, n, n)
    counts_d = engine.dev(counts, torch.int64)
    q = posterior.QUANTILES
    res = {'samples': n, 'expansion': total,
           'regime': 'resident' if n <= _capi.lib().pb_weighted_quantiles_resident_rows()
           else 'streaming'}
    state = Sampler()
    got = posterior.weighted_quantiles(store, counts_d, q, total=total)
    with state:
        res['kernel_ms'] = device_ms(
            lambda: posterior.weighted_quantiles(store, counts_d, q, total=total), args.steps,
            args.warmup)
    res['gpu_state'] = state.summary()
    nbytes = 8.0 * nwave * n
    res['store_GB'] = round(nbytes / 1e9, 2)
    res['kernel_GBps'] = round(nbytes / (res['kernel_ms'] * 1e-3) / 1e9, 1)
    res['traffic_bound_ms'] = nbytes / (hbm_gbps * 1e9) * 1e3
    res['fraction_of_traffic_bound'] = res['traffic_bound_ms'] / res['kernel_ms']
    lo, hi, gamma = (engine.dev(x, dt) for x, dt in zip(
        posterior.quantile_ranks(total, q), (torch.int64, torch.int64, torch.float64)))
    alt = torch_route(store, counts_d, lo, hi, gamma, args.block)
    res['torch_route_ms'] = device_ms(
        lambda: torch_route(store, counts_d, lo, hi, gamma, args.block), max(args.steps // 3, 1), 0)
    res['torch_route_over_kernel'] = res['torch_route_ms'] / res['kernel_ms']
    res['torch_route_equal_bits'] = bool(torch.equal(alt, got))
    cols = min(args.host_columns, nwave)
    inverse = rng.permutation(np.repeat(np.arange(n), counts))
    seconds, want = host_route(store, inverse, 100 * np.array(q), cols)
    res['host_route_columns'] = cols
    res['host_route_ms_scaled'] = 1e3 * seconds * nwave / cols
    res['host_route_over_kernel'] = res['host_route_ms_scaled'] / res['kernel_ms']
    res['host_route_equal_bits'] = bool(np.array_equal(got[:, :cols].cpu().numpy(), want))
    del store, alt, got
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--samples', default='4096,32768')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--nwave', type=int, default=bench_c5.NWAVE)
    ap.add_argument('--block', type=int, default=8192, help='columns per block of torch_route')
    ap.add_argument('--host-columns', type=int, default=64)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    box = bench_c5.box_reference()
    res = {'workload': 'c5-posterior', 'steps': args.steps, 'nwave': args.nwave,
           'quantiles': 5, 'box_reference': box}
    for n in (int(v) for v in args.samples.split(',')):
        res[f'n{n}'] = run(n, args.nwave, args, box['copy_GBps'])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
