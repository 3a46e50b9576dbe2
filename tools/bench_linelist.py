#!/usr/bin/env python3
"""Line lists to TLI columns on the device (pyratbay_amd/linelist.py, csrc/pb_linelist.hip):

  * the parse kernels alone (pb_parse_hitran, pb_parse_exomol): records/s and bytes/s of text,
    beside a device-to-device copy of the same bytes timed in the same session, alternating;
  * the whole device route of make_tli from a file (page cache) through the two pinned buffers
    to sorted host columns and the written file, with its stages: the file read alone, the
    read + copy + parse + gf + filter of _read_device, the sort;
  * the host route (device=False) on the same text, at the small size only.

Input: synthetic text generated in memory from a seed -- the mock HITRAN records of
tests/golden repeated with rising wavenumbers, and ExoMol transitions over a synthetic states
table.  Medians of --reps runs with min and max.  Numbers: profiles/linelist.md.

    python tools/bench_linelist.py [--records 1000000,10000000] [--exomol 10000000]
                                   [--states 1000000] [--reps 7] [--out result.json]
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
G32 = os.path.join(ROOT, 'tests', 'golden', 'g32_linelist.npz')


def put_digits(out, col0, values, ndigits):
    """ASCII digits of the integers `values`, right-aligned in columns col0 .. col0+ndigits-1."""
    v = values.copy()
    for k in range(ndigits - 1, -1, -1):
        out[:, col0 + k] = 48 + (v % 10)
        v //= 10


def hitran_text(n, seed=1):
    """n records [n, 162] uint8: the mock records repeated, wavenumbers rising by 1e-3 cm-1 from
    1000 (F12.6), Elow perturbed in its last digits."""
    rng = np.random.default_rng(seed)
    base = np.load(G32)['input_Mock_HITRAN_H2O_1.00-1.01um.par'].reshape(-1, 162)
    text = base[np.arange(n) % len(base)].copy()
    micro = 1_000_000_000 + 1000 * np.arange(n, dtype=np.int64)         # wn * 1e6
    put_digits(text, 3, micro // 1_000_000, 5)
    text[:, 8] = ord('.')
    put_digits(text, 9, micro % 1_000_000, 6)
    put_digits(text, 52, rng.integers(0, 1000, n), 3)                    # Elow's last digits
    return text


def exomol_text(n, nstates, seed=2):
    """(text [n, 37] uint8, energy, degeneracy): `%12d %12d %10.4e\\n` records, upper state
    above the lower one, sorted by wavenumber like a .trans file."""
    rng = np.random.default_rng(seed)
    energy = np.round(np.sort(rng.uniform(0.0, 20000.0, nstates)), 6)
    degeneracy = rng.integers(1, 400, nstates).astype(np.float64)
    low = rng.integers(0, nstates - 1, n)
    up = np.minimum(low + 1 + rng.integers(0, nstates // 4, n), nstates - 1)
    order = np.argsort(energy[up] - energy[low], kind='stable')
    up, low = up[order], low[order]
    pool = np.array([list(f'{10.0 ** rng.uniform(-12, 2):10.4e}'.encode())
                     for _ in range(4096)], np.uint8)
    text = np.full((n, 37), 32, np.uint8)
    put_digits(text, 0, up, 12)
    put_digits(text, 13, low, 12)
    for col in (0, 13):                                                  # leading zeros to blanks
        lead = np.cumsum(text[:, col:col + 11] != 48, axis=1) == 0
        text[:, col:col + 11][lead] = 32
    text[:, 26:36] = pool[rng.integers(0, 4096, n)]
    text[:, 36] = 10
    return text, energy, degeneracy


def stats(samples):
    s = sorted(samples)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def time_device(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def bench_kernel(kind, text, reps, states=None):
    """Seconds of the parse kernel and of a device-to-device copy of its text, alternating."""
    import torch
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
    n, recsize = text.shape
    text_d = torch.from_numpy(text.reshape(-1)).cuda()
    copy_d = torch.empty_like(text_d)
    cols = [torch.empty(n, dtype=torch.float64, device='cuda') for _ in range(4)]
    iso = torch.empty(n, dtype=torch.int16, device='cuda')
    flags = torch.empty(n, dtype=torch.uint8, device='cuda')
    count = torch.zeros(1, dtype=torch.int32, device='cuda')
    out = [_ptr(c) for c in cols] + [_ptr(iso), _ptr(flags), _ptr(count)]
    if kind == 'hitran':
        def parse():
            call('pb_parse_hitran', _ptr(text_d), n, recsize, *out, _stream())
    else:
        e_d, g_d = (torch.from_numpy(a).cuda() for a in states)

        def parse():
            call('pb_parse_exomol', _ptr(text_d), n, recsize, _ptr(e_d), _ptr(g_d),
                 len(states[0]), 0, *out, _stream())
    gf = torch.empty(n, dtype=torch.float64, device='cuda')

    def gf_kernel():
        call('pb_linelist_gf', _ptr(cols[0]), _ptr(cols[2]), _ptr(cols[3]), n, 1.0, 1.0,
             _ptr(gf), _stream())
    t_parse, t_copy, t_gf = [], [], []
    for _ in range(reps):
        t_parse += time_device(parse, 1)
        t_copy += time_device(lambda: copy_d.copy_(text_d), 1)
        t_gf += time_device(gf_kernel, 1)
    nbytes = n * recsize
    p, c = stats(t_parse), stats(t_copy)
    return dict(kind=kind, records=n, recsize=recsize, flagged=int(count.item()) // (reps * 2),
                parse_s=p, copy_s=c, gf_s=stats(t_gf),
                records_per_s=n / p['median'], text_bytes_per_s=nbytes / p['median'],
                # what the kernel moves: the text once, 4 doubles + int16 + uint8 out
                moved_bytes_per_s=(nbytes + n * 35) / p['median'],
                copy_bytes_per_s=2 * nbytes / c['median'],
                parse_over_copy=p['median'] / c['median'])


def bench_route(ll, db, nrec, reps, chunk_bytes, tmp):
    """make_tli from the file to the written TLI, and its stages."""
    import torch
    file = db.files[0]
    out = os.path.join(tmp, 'bench.tli')
    whole, read, parse, sort = [], [], [], []
    pinned = torch.empty(chunk_bytes, dtype=torch.uint8).pin_memory()
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        ll.make_tli(db, out, wn_low=-np.inf, wn_high=np.inf, device=True,
                    chunk_bytes=chunk_bytes)
        t1 = time.perf_counter()
        with open(file.path, 'rb') as f:
            view = memoryview(pinned.numpy())
            while f.readinto(view):
                pass
        t2 = time.perf_counter()
        chunker = ll._Chunker(chunk_bytes)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        wn, gf, elow, iso = ll._read_device(db, file, 0, nrec - 1, chunker)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        order = torch.sort(wn, stable=True)[1]
        order = order[torch.sort(iso[order], stable=True)[1]]
        cols = [t[order].cpu() for t in (wn, gf, elow, iso)]
        t5 = time.perf_counter()
        del chunker, wn, gf, elow, iso, order, cols
        if rep:                                                          # the first one warms up
            whole.append(t1 - t0)
            read.append(t2 - t1)
            parse.append(t4 - t3)
            sort.append(t5 - t4)
    w = stats(whole)
    return dict(records=nrec, chunk_bytes=chunk_bytes, make_tli_s=w,
                records_per_s=nrec / w['median'], file_read_s=stats(read),
                read_copy_parse_gf_s=stats(parse), sort_download_s=stats(sort),
                flagged=ll.last_flagged())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', default='1000000,10000000')
    ap.add_argument('--exomol', type=int, default=10_000_000)
    ap.add_argument('--states', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--chunk-bytes', type=int, default=256 << 20)
    ap.add_argument('--host-records', type=int, default=1_000_000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from pyratbay_amd import linelist as ll
    from pyratbay_amd import _device
    _device.require_gpu()
    g = np.load(G32)
    result = dict(device=torch.cuda.get_device_name(0), kernels=[], routes=[])
    with tempfile.TemporaryDirectory() as tmp:
        for n in [int(x) for x in args.records.split(',') if x]:
            text = hitran_text(n)
            result['kernels'].append(bench_kernel('hitran', text, args.reps))
            path = os.path.join(tmp, f'synthetic_{n}.par')
            text.tofile(path)
            db = ll.Hitran(path, molecule='H2O', isotopes=list(g['h2o_isotopes']),
                           iso_mass=g['h2o_mass'], iso_ratio=g['h2o_ratio'],
                           partition=(g['h2o_pf_temp'], g['h2o_pf'],
                                      list(g['h2o_pf_isotopes'])))
            result['routes'].append(bench_route(ll, db, n, max(3, args.reps // 2),
                                                args.chunk_bytes, tmp))
            if n == args.host_records:
                t0 = time.perf_counter()
                ll.make_tli(db, os.path.join(tmp, 'host.tli'), wn_low=-np.inf, wn_high=np.inf,
                            device=False)
                result['host_route'] = dict(records=n, make_tli_s=time.perf_counter() - t0)
                with open(os.path.join(tmp, 'host.tli'), 'rb') as f, \
                        open(os.path.join(tmp, 'bench.tli'), 'rb') as h:
                    result['host_route']['same_bytes_as_device'] = f.read() == h.read()
            os.remove(path)
            print(json.dumps(result['kernels'][-1]), flush=True)
            print(json.dumps(result['routes'][-1]), flush=True)
        if args.exomol:
            text, energy, degeneracy = exomol_text(args.exomol, args.states)
            result['kernels'].append(bench_kernel('exomol', text, args.reps,
                                                  (energy, degeneracy)))
            print(json.dumps(result['kernels'][-1]), flush=True)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
