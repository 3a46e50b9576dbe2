#!/usr/bin/env python3
"""Partition functions from ExoMol states on the device (pyratbay_amd/partitions.py,
csrc/pb_partitions.hip):

  * pb_pf_states (k_pf_states + k_pf_reduce) alone: ms, terms/s and the fraction of the FP64
    vector rate that the term's instruction count implies, beside the same tensors through the
    chunked torch expression (g[:, None] * torch.exp(-C2 * E[:, None] / T)).sum(0), in the same
    process, timed alternately, and the largest relative difference of the two results;
  * pb_parse_states beside a device-to-device copy of its text, alternately;
  * exomol_states end to end from a file in the page cache, and device=False at a small size;
  * linelist.read_states on the device and on the host.

Input: synthetic states generated in memory from a seed (`%12d %12.6f %6d` and quantum numbers,
86-byte records), 1000 temperatures (5 ... 5000 K in steps of 5 K).  Medians of --reps runs with
min and max.  Numbers: profiles/partitions.md.

    python tools/bench_partitions.py [--states 1000000,10000000] [--reps 7]
                                     [--host-states 100000] [--read-states 1000000]
                                     [--out result.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECSIZE = 86
GRID = (5.0, 5000.0, 5.0)
# Vector instructions of k_pf_states per (state, temperature) term, counted in the ISA of the
# inner loop (gfx950, the build's flags): the argument's product, exp (a product, v_rndne, two
# fma of the reduction, eleven fma of the polynomial, two of the reconstruction, v_cvt_i32,
# v_ldexp, two compares and three v_cndmask of the range checks) and the fma into the sum: 26,
# of which 22 are FP64 operations; per state one more product and two moves, shared by the four
# temperatures of a lane.
VALU_PER_TERM = 26.75
# FP64 vector rate of the part: 78.6 TFLOPS counts an fma as two, so 39.3e12 lane-operations/s
# (16 lanes per SIMD and clock at 2.4 GHz: a wavefront instruction takes four clocks)
FP64_LANE_OPS_PER_S = 39.3e12


def put_digits(out, col0, values, ndigits):
    """ASCII digits of the integers `values`, right-aligned in columns col0 .. col0+ndigits-1."""
    v = values.copy()
    for k in range(ndigits - 1, -1, -1):
        out[:, col0 + k] = 48 + (v % 10)
        v //= 10


def blank_leading_zeros(text, col0, ndigits):
    lead = np.cumsum(text[:, col0:col0 + ndigits - 1] != 48, axis=1) == 0
    text[:, col0:col0 + ndigits - 1][lead] = 32


def states_text(n, seed=3):
    """(text [n, 86] uint8, energy, degeneracy): ids 1 .. n, energies rising from 0 to 40000
    cm-1 (`%12.6f`), degeneracies 1 .. 399."""
    rng = np.random.default_rng(seed)
    micro = np.sort(rng.integers(0, 40_000_000_000, n))               # energy * 1e6
    micro[0] = 0
    g = rng.integers(1, 400, n)
    text = np.full((n, RECSIZE), 32, np.uint8)
    put_digits(text, 0, np.arange(1, n + 1, dtype=np.int64), 12)
    blank_leading_zeros(text, 0, 12)
    put_digits(text, 13, micro // 1_000_000, 5)
    blank_leading_zeros(text, 13, 5)
    text[:, 18] = ord('.')
    put_digits(text, 19, micro % 1_000_000, 6)
    put_digits(text, 26, g, 6)
    blank_leading_zeros(text, 26, 6)
    tail = np.frombuffer(b'       0   1.6537E-01      +   e   0   0   2   0   0', np.uint8)
    text[:, 32:32 + len(tail)] = tail
    text[:, RECSIZE - 1] = 10
    return text, micro / 1e6, g.astype(np.float64)


def stats(samples):
    s = sorted(samples)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def time_device(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def torch_expression(energy, g, temps, c2, chunk):
    import torch
    q = torch.zeros_like(temps)
    for a in range(0, energy.numel(), chunk):
        e, w = energy[a:a + chunk], g[a:a + chunk]
        q += (w[:, None] * torch.exp(-c2 * e[:, None] / temps)).sum(0)
    return q


def bench_pf(pf, energy, g, reps, chunk):
    import torch
    e_d, g_d = torch.from_numpy(energy).cuda(), torch.from_numpy(g).cuda()
    t_d = torch.from_numpy(pf.temperature_grid(*GRID)).cuda()
    n, ntemp = e_d.numel(), t_d.numel()
    got = pf.states_partition(e_d, g_d, t_d)                           # warm up both
    want = torch_expression(e_d, g_d, t_d, pf.C2, chunk)
    torch.cuda.synchronize()
    t_kernel, t_torch = [], []
    for _ in range(reps):
        t_kernel.append(time_device(lambda: pf.states_partition(e_d, g_d, t_d)))
        t_torch.append(time_device(lambda: torch_expression(e_d, g_d, t_d, pf.C2, chunk)))
    k, b = stats(t_kernel), stats(t_torch)
    terms = n * ntemp
    return dict(states=n, temperatures=ntemp, terms=terms, pf_states_s=k, torch_expression_s=b,
                torch_chunk=chunk, terms_per_s=terms / k['median'],
                fp64_issue_floor_s=terms * VALU_PER_TERM / FP64_LANE_OPS_PER_S,
                fraction_of_fp64_vector_rate=terms * VALU_PER_TERM / FP64_LANE_OPS_PER_S
                / k['median'],
                torch_over_kernel=b['median'] / k['median'],
                max_rel_difference=float(((got - want).abs() / want).max()))


def bench_parse(text, reps):
    import torch
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
    n, recsize = text.shape
    text_d = torch.from_numpy(text.reshape(-1)).cuda()
    copy_d = torch.empty_like(text_d)
    ids = torch.empty(n, dtype=torch.int64, device='cuda')
    e, g = (torch.empty(n, dtype=torch.float64, device='cuda') for _ in range(2))
    flags = torch.empty(n, dtype=torch.uint8, device='cuda')
    count = torch.zeros(1, dtype=torch.int32, device='cuda')

    def parse():
        call('pb_parse_states', _ptr(text_d), n, recsize, _ptr(ids), _ptr(e), _ptr(g),
             _ptr(flags), _ptr(count), _stream())
    parse()
    copy_d.copy_(text_d)
    torch.cuda.synchronize()
    t_parse, t_copy = [], []
    for _ in range(reps):
        t_parse.append(time_device(parse))
        t_copy.append(time_device(lambda: copy_d.copy_(text_d)))
    p, c = stats(t_parse), stats(t_copy)
    return dict(records=n, recsize=recsize, flagged=int(count.item()) // (reps + 1), parse_s=p,
                copy_s=c, records_per_s=n / p['median'], text_bytes_per_s=n * recsize / p['median'],
                parse_over_copy=p['median'] / c['median'])


def bench_route(pf, path, n, reps):
    import torch
    whole = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        pf.exomol_states(path, *GRID)
        torch.cuda.synchronize()
        if rep:
            whole.append(time.perf_counter() - t0)
    w = stats(whole)
    return dict(states=n, exomol_states_s=w, states_per_s=n / w['median'],
                flagged=pf.last_flagged())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--states', default='1000000,10000000')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-states', type=int, default=100_000)
    ap.add_argument('--read-states', type=int, default=1_000_000)
    ap.add_argument('--torch-chunk', type=int, default=32768)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import contextlib
    import io
    import torch
    from pyratbay_amd import _device
    from pyratbay_amd import linelist as ll
    from pyratbay_amd import partitions as pf
    _device.require_gpu()
    result = dict(device=torch.cuda.get_device_name(0), pf=[], parse=[], routes=[])
    quiet = contextlib.redirect_stdout(io.StringIO())
    with tempfile.TemporaryDirectory() as tmp:
        for n in [int(x) for x in args.states.split(',') if x]:
            text, energy, g = states_text(n)
            result['pf'].append(bench_pf(pf, energy, g, args.reps if n <= 2_000_000 else 3,
                                         args.torch_chunk))
            print(json.dumps(result['pf'][-1]), flush=True)
            result['parse'].append(bench_parse(text, args.reps))
            print(json.dumps(result['parse'][-1]), flush=True)
            path = os.path.join(tmp, f'1H-12C-14N__Synthetic{n}.states')
            text.tofile(path)
            with quiet:
                result['routes'].append(bench_route(pf, path, n, 3))
            print(json.dumps(result['routes'][-1]), flush=True)
            if n == args.read_states:
                t_dev, t_host = [], []
                ll.read_states(path, device=True)
                for _ in range(3):
                    t0 = time.perf_counter()
                    dev = ll.read_states(path, device=True)
                    t1 = time.perf_counter()
                    host = ll.read_states(path)
                    t2 = time.perf_counter()
                    t_dev.append(t1 - t0)
                    t_host.append(t2 - t1)
                result['read_states'] = dict(
                    states=n, device_s=stats(t_dev), host_s=stats(t_host),
                    same_arrays=bool(np.array_equal(dev[0].view(np.uint64),
                                                    host[0].view(np.uint64))
                                     and np.array_equal(dev[1], host[1])))
                print(json.dumps(result['read_states']), flush=True)
            os.remove(path)
        if args.host_states:
            n = args.host_states
            text, energy, g = states_text(n)
            path = os.path.join(tmp, f'1H-12C-14N__Synthetic{n}.states')
            text.tofile(path)
            t_dev, t_host = [], []
            with quiet:
                pf.exomol_states(path, *GRID)
                for _ in range(3):
                    t0 = time.perf_counter()
                    dev = pf.exomol_states(path, *GRID)[0]
                    t1 = time.perf_counter()
                    host = pf.exomol_states(path, *GRID, device=False)[0]
                    t2 = time.perf_counter()
                    t_dev.append(t1 - t0)
                    t_host.append(t2 - t1)
            result['host_route'] = dict(states=n, device_s=stats(t_dev), host_s=stats(t_host),
                                        max_rel_difference=float(np.max(np.abs(dev / host - 1))))
            print(json.dumps(result['host_route']), flush=True)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
