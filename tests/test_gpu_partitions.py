"""Partition functions on the device: pb_parse_states against its host statement bit for bit,
pb_pf_states against exact arithmetic within the bound of partitions_cases.rel_bound, and
exomol_states / read_states (device=True) against the host route."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import linelist_cases as lc
import partitions_cases as pc
from pyratbay_amd import linelist as ll
from pyratbay_amd import partitions as pf
from pyratbay_amd import tli

pytestmark = pytest.mark.gpu
GUARD = 64                                     # elements in front of and behind every output
OFFSETS = (0, 1, 7, 15)


def _constant(name):
    from pyratbay_amd import _capi
    return _capi.constant(name)


def _guarded(n, dtype, fill):
    import torch
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda')


def _check_guards(buf, n, fill):
    host = buf.cpu().numpy()
    guard = np.concatenate([host[:GUARD], host[GUARD + n:]])
    if host.dtype == np.float64:
        assert np.all(np.isnan(guard))
    else:
        assert np.all(guard == fill)
    return host[GUARD:GUARD + n].copy()


def _parse(data, nrec, recsize, offset=0):
    """One launch of pb_parse_states at the kernel boundary: text_d `offset` bytes behind a
    16-byte boundary, every output inside a larger buffer filled with NaN / 0x7f whose guard
    elements must come back untouched."""
    import torch
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
    raw = np.frombuffer(bytes(data[:nrec * recsize]), np.uint8)
    text = torch.full((offset + len(raw) + 16,), 0x7f, dtype=torch.uint8, device='cuda')
    assert text.data_ptr() % 16 == 0
    text[offset:offset + len(raw)] = torch.from_numpy(raw.copy()).cuda()
    ids = _guarded(nrec, torch.int64, 0x7f7f7f7f7f7f7f7f)
    energy = _guarded(nrec, torch.float64, float('nan'))
    g = _guarded(nrec, torch.float64, float('nan'))
    flags = _guarded(nrec, torch.uint8, 0x7f)
    count = torch.zeros(3, dtype=torch.int32, device='cuda')
    call('pb_parse_states', _ptr(text[offset:]), nrec, recsize,
         *(_ptr(b[GUARD:GUARD + nrec]) for b in (ids, energy, g, flags)), _ptr(count[1:2]),
         _stream())
    torch.cuda.synchronize()
    counts = count.cpu().numpy()
    assert counts[0] == 0 and counts[2] == 0
    return (_check_guards(ids, nrec, 0x7f7f7f7f7f7f7f7f), _check_guards(energy, nrec, None),
            _check_guards(g, nrec, None), _check_guards(flags, nrec, 0x7f), int(counts[1]))


def _assert_parse(got, host, n):
    ids, energy, g, flags, count = got
    assert np.array_equal(ids, host[0][:n])
    assert pc.same_columns(energy, host[1][:n]) and pc.same_columns(g, host[2][:n])
    assert np.array_equal(flags, host[3][:n])
    assert count == np.count_nonzero(host[3][:n])


def _crafted_records(recsize, n):
    """n records: seeded clean ones, the constructed flagged and clean forms among the first 63
    and again in the second and third workgroup."""
    rng = np.random.default_rng(recsize)
    records = [pc.random_states(rng, 1, recsize, first_id=100 + i) for i in range(n)]
    for base in (0, 131, n - 41):
        for k, (_, head, _) in enumerate(pc.FLAGGED):
            records[base + 2 * k + 1] = pc.flagged_record(head, recsize)
        records[base + 29] = pc.short_line(recsize)
        for k, head in enumerate(pc.CLEAN):
            records[base + 30 + k] = pc.flagged_record(head, recsize)
    return records


@pytest.mark.parametrize('recsize', [33, 86, 139, 255])
def test_parse_states_equals_the_host_statement(recsize):
    """Flags and flagged count included; one lane, one wavefront, one workgroup, each with one
    record more and one fewer, and two workgroups and a record; text at byte offsets 0, 1, 7, 15
    from a 16-byte boundary; guards untouched."""
    W = _constant('PB_STATES_RECORDS_PER_BLOCK')
    sizes = (0, 1, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1)
    data = b''.join(_crafted_records(recsize, max(sizes)))
    host = pf.parse_states_host(data, recsize)
    want = np.zeros(max(sizes), bool)
    for base in (0, 131, max(sizes) - 41):
        want[base + 1:base + 2 * len(pc.FLAGGED):2] = True
        want[base + 29] = True
    assert np.array_equal(host[3] != 0, want)                  # exactly the constructed set
    for n in sizes:
        for offset in OFFSETS:
            _assert_parse(_parse(data, n, recsize, offset), host, n)


@pytest.mark.parametrize('file', pc.NH3 + pc.HCN)
def test_parse_states_on_the_fixture_files(file):
    with open(file, 'rb') as f:
        data = f.read()
    recsize = pc.RECSIZE[file]
    host = pf.parse_states_host(data, recsize)
    n = len(data) // recsize
    got = _parse(data, n, recsize, offset=7)
    _assert_parse(got, host, n)
    assert got[4] == 0
    e, g = pc.fixture_states(pf, file)
    assert np.array_equal(pc.bits(got[1]), pc.bits(e)) and np.array_equal(got[2], g)


# ---------------------------------------------------------------------------------------------
# pb_pf_states
# ---------------------------------------------------------------------------------------------
def _work_sizes(nstates, ntemp):
    from pyratbay_amd._capi import call
    sizes = (ctypes.c_int64 * 2)()
    call('pb_pf_states_work', nstates, ntemp, sizes)
    return int(sizes[0]), int(sizes[1])


def _pf(energy, g, temps, stream=None):
    """One pb_pf_states at the kernel boundary: q_d and work_d inside NaN-filled buffers whose
    guard elements must come back untouched."""
    import torch
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
    nstates, ntemp = len(energy), len(temps)
    nwork, _ = _work_sizes(nstates, ntemp)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        e_d = torch.from_numpy(np.asarray(energy, np.float64).copy()).cuda()
        g_d = torch.from_numpy(np.asarray(g, np.float64).copy()).cuda()
        t_d = torch.from_numpy(np.asarray(temps, np.float64).copy()).cuda()
        q = _guarded(ntemp, torch.float64, float('nan'))
        work = _guarded(nwork, torch.float64, float('nan'))
        call('pb_pf_states', _ptr(e_d) if nstates else None, _ptr(g_d) if nstates else None,
             nstates, _ptr(t_d), ntemp, pf.C2, _ptr(q[GUARD:GUARD + ntemp]),
             _ptr(work[GUARD:GUARD + max(nwork, 1)]), _stream())
    torch.cuda.synchronize()
    _check_guards(work, nwork, None)
    return _check_guards(q, ntemp, None)


_master = {}


def _master_case():
    """2C + 1 states (the first with E = 0, every seventh with g = 0) and Tt + 1 temperatures from
    20 K to 6000 K; the exact terms at six of the temperatures, summed once over every prefix."""
    if not _master:
        C = _work_sizes(1, 1)[1]
        Tt = _constant('PB_PF_TEMPS_PER_TILE')
        rng = np.random.default_rng(1033)
        n = 2 * C + 1
        energy = np.round(rng.uniform(0.0, 30000.0, n), 6)
        energy[0] = 0.0
        g = rng.integers(1, 400, n).astype(np.float64)
        g[6::7] = 0.0
        temps = np.geomspace(20.0, 6000.0, Tt + 1)
        at = [0, 62, 63, 64, Tt - 1, Tt]
        import decimal
        prefix = []                                            # prefix[k][n]: states 0 .. n-1
        for t in at:
            sums, total = [decimal.Decimal(0)], decimal.Decimal(0)
            for j in range(n):
                total = pc.CONTEXT.add(
                    total, pc.exact_q(energy[j:j + 1], g[j:j + 1], [temps[t]], pf.C2)[0])
                sums.append(total)
            prefix.append(sums)
        _master.update(C=C, Tt=Tt, energy=energy, g=g, temps=temps, at=at, prefix=prefix)
    return _master


def test_pf_states_sizes_tiles_and_chunks():
    """Every pair of nstates in {0, 1, 63, 64, 65, C-1, C, C+1, 2C+1} and ntemp in {1, 63, 64, 65,
    Tt+1}: within twice the bound of the 50-digit sum at the first and last temperatures and
    around the wavefront boundary, and within the summed allowances of the host statement at all
    of them."""
    m = _master_case()
    C, Tt = m['C'], m['Tt']
    assert C == _constant('PB_PF_MIN_CHUNK')
    for n in (0, 1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1):
        assert _work_sizes(n, 7) == (7 * -(-n // C), C)
        e, g = m['energy'][:n], m['g'][:n]
        host = pf.states_partition_host(e, g, m['temps'])
        bound = pc.rel_bound(e, g, m['temps'], pf.C2)
        for ntemp in (1, 63, 64, 65, Tt + 1):
            got = _pf(e, g, m['temps'][:ntemp])
            if n == 0:
                assert np.all(got == 0.0) and not np.signbit(got).any()
                continue
            pc.assert_close(got, host[:ntemp], bound[:ntemp], bound[:ntemp], n, (n, ntemp))
            at = [k for k, t in enumerate(m['at']) if t < ntemp]
            idx = [m['at'][k] for k in at]
            pc.assert_q(got[idx], [m['prefix'][k][n] for k in at], bound[idx], n, (n, ntemp))


def test_pf_states_underflow_denormals_and_empty_states():
    # 1 K and energies of 1e4 cm-1 and above: every term underflows
    energy = 1e4 + np.arange(100.0)
    g = np.full(100, 7.0)
    got = _pf(energy, g, [1.0])
    pc.assert_q(got, pc.exact_q(energy, g, [1.0], pf.C2), [1.0], 100)
    assert got[0] == 0.0
    # x = 725 ... 740: every term is a denormal, and so is their sum
    t = pf.C2 * 1e4 / 725.0
    energy = 1e4 * np.linspace(1.0, 740.0 / 725.0, 50)
    g = np.ones(50)
    exact = pc.exact_q(energy, g, [t], pf.C2)
    assert 0 < exact[0] < 50 * pc.TINY
    got = _pf(energy, g, [t])
    pc.assert_q(got, exact, [1.0], 50)
    assert got[0] > 0.0                                        # denormals are kept
    # one normal term (x = 700) above them: the whole bound holds
    energy = np.concatenate([[1e4 * 700.0 / 725.0], energy])
    g = np.ones(51)
    exact = pc.exact_q(energy, g, [t], pf.C2)
    assert exact[0] > 51 * pc.TINY
    pc.assert_q(_pf(energy, g, [t]), exact, pc.rel_bound(energy, g, [t], pf.C2), 51)
    # only empty states: zero
    assert np.all(_pf(np.zeros(65), np.zeros(65), [10.0, 300.0]) == 0.0)
    # no temperature: no launch, nothing written
    assert len(_pf(np.ones(3), np.ones(3), [])) == 0


def test_pf_states_same_bits_on_every_call_and_stream():
    import torch
    m = _master_case()
    first = _pf(m['energy'], m['g'], m['temps'])
    again = _pf(m['energy'], m['g'], m['temps'])
    other = _pf(m['energy'], m['g'], m['temps'], stream=torch.cuda.Stream())
    assert np.array_equal(pc.bits(first), pc.bits(again))
    assert np.array_equal(pc.bits(first), pc.bits(other))


def test_states_partition_refuses_what_it_does_not_take():
    import torch
    e = torch.zeros(4, dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='4 energies and 3 degeneracies'):
        pf.states_partition(e, e[:3], e)
    with pytest.raises(ValueError, match='temps must be a 1D device tensor of doubles'):
        pf.states_partition(e, e, e.cpu())
    q = pf.states_partition(e[:0], e[:0], torch.ones(5, dtype=torch.float64, device='cuda'))
    assert q.shape == (5,) and bool((q == 0).all())


# ---------------------------------------------------------------------------------------------
# exomol_states, read_states
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mol', ['nh3', 'hcn'])
def test_exomol_states_device_against_the_host_route(mol, tmp_path):
    """On the fixture files: within the summed bounds of device=False and of the reference's
    arrays, within the bound of the exact sums, nothing flagged, the reference's file."""
    g33 = pc.g33()
    out = str(tmp_path / 'PF.dat')
    for grid in ('a', 'b'):
        args = pc.GRIDS[grid]
        q, isotopes, temps = pf.exomol_states(pc.STATES[mol], *args, outfile=out)
        assert pf.last_flagged() == 0 and pf.routes() == ['device'] * len(pc.STATES[mol])
        host = pf.exomol_states(pc.STATES[mol], *args, device=False)
        assert isotopes == host[1] and np.array_equal(pc.bits(temps), pc.bits(host[2]))
        for i, file in enumerate(pc.STATES[mol]):
            e, g = pc.fixture_states(pf, file)
            bound = pc.rel_bound(e, g, temps, pf.C2)
            pc.assert_close(q[i], host[0][i], bound, bound, len(e), file)
            pc.assert_close(q[i], g33[f'states_{mol}_{grid}_pf'][i], bound, bound, len(e), file)
            if grid == 'b':
                at = [int(np.nonzero(temps == t)[0][0]) for t in pc.EXACT_TEMPS]
                pc.assert_q(q[i, at], pc.fixture_exact(pf, file), bound[at], len(e), file)
        with open(out, 'rb') as f:
            assert f.read() == g33[f'states_{mol}_{grid}_file'].tobytes()


def _crafted_file(tmp_path, name, ragged=False):
    """A `.states` file of 600 records with id gaps, three flagged records that the host reads
    (an exponent beyond the fast path, a tab, an energy outside its columns) and, if ragged, one
    line a byte shorter."""
    rng = np.random.default_rng(7)
    lines = []
    for i in range(600):
        ident = 1 + i + (i // 50) * 3                          # gaps of three ids
        lines.append(pc.states_record(ident, f'{rng.uniform(0, 9000):.6f}',
                                      int(rng.integers(1, 99)), 86))
    lines[123] = pc.states_record(lines[123].split()[0].decode(), '1.25e+25', 5, 86)
    lines[456] = pc.flagged_record(f'{2000:>12} {"12.5":>12}\t{3:>5}', 86)
    # the layout flag with the line feed in place: the energy starts before byte 12 (the `pf`
    # reading, bytes 12 ... 31, then takes .875419, as the reference does)
    lines[200] = pc.flagged_record(f'{1999:>9} {"30.875419":<12} {18:>8}', 86)
    if ragged:
        lines[300] = lines[300][:-2] + b'\n'
    path = str(tmp_path / name)
    with open(path, 'wb') as f:
        f.write(b''.join(lines))
    return path


def test_exomol_states_flagged_records_chunks_and_ragged_lines(tmp_path):
    args = (50.0, 3000.0, 50.0)
    path = _crafted_file(tmp_path, '1H-12C-14N__Crafted.states')
    host = pf.exomol_states(path, *args, device=False)[0]
    e, g = pf.read_states_pf_host(path)
    bound = pc.rel_bound(e, g, pf.temperature_grid(*args), pf.C2)
    for chunk_bytes in (256 << 20, 100 * 86 + 7):              # one chunk; six, both buffers
        q = pf.exomol_states(path, *args, chunk_bytes=chunk_bytes)[0]
        assert pf.last_flagged() == 3 and pf.routes() == ['device']
        pc.assert_close(q[0], host[0], bound, bound, len(e), chunk_bytes)
    # lines of two lengths: the host route, the host's bits
    ragged = _crafted_file(tmp_path, '1H-12C-15N__Ragged.states', ragged=True)
    host = pf.exomol_states(ragged, *args, device=False)[0]
    q = pf.exomol_states(ragged, *args)[0]
    assert pf.last_flagged() == 0 and pf.routes() == ['host']
    assert np.array_equal(pc.bits(q), pc.bits(host))
    assert pf.parse_states_device(ragged) is None
    # a line feed in the wrong place of a file whose size is a multiple of the record size
    with open(ragged, 'ab') as f:
        f.write(b' ')
    assert os.path.getsize(ragged) % 86 == 0 and pf.parse_states_device(ragged) is None


def test_bz2_states_take_the_device_route(tmp_path):
    """`.states.bz2` is decompressed on the host and parsed on the device: the bits of the plain
    file's device route, for the fixture and for the file with flagged records."""
    import bz2
    args = (50.0, 3000.0, 50.0)
    for plain in (pc.HCN[0], _crafted_file(tmp_path, '1H-12C-14N__Crafted.states')):
        os.makedirs(tmp_path / 'packed', exist_ok=True)
        packed = str(tmp_path / 'packed' / (os.path.basename(plain) + '.bz2'))
        with open(plain, 'rb') as f, bz2.open(packed, 'wb') as z:
            z.write(f.read())
        want = pf.exomol_states(plain, *args, chunk_bytes=100 * 86)[0]
        flagged = pf.last_flagged()
        assert pf.routes() == ['device'] and flagged == (0 if plain == pc.HCN[0] else 3)
        got = pf.exomol_states(packed, *args, chunk_bytes=100 * 86)[0]
        assert pf.routes() == ['device'] and pf.last_flagged() == flagged
        assert np.array_equal(pc.bits(got), pc.bits(want))
        dense, dense_bz2 = ll.read_states(plain, device=True), ll.read_states(
            packed[:-4], device=True)
        assert np.array_equal(pc.bits(dense[0]), pc.bits(dense_bz2[0]))
        assert np.array_equal(dense[1], dense_bz2[1])


def test_read_states_device_equals_the_host_route(tmp_path):
    for file in pc.NH3 + pc.HCN:
        want = ll.read_states(file)
        assert pf.parse_states_device(file, 'states') is not None
        got = ll.read_states(file, device=True)
        assert pf.last_flagged() == 0
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(pc.bits(got[0]), pc.bits(want[0]))
        assert np.array_equal(got[1], want[1])
    path = _crafted_file(tmp_path, '1H-12C-14N__Crafted.states')
    want = ll.read_states(path)
    got = ll.read_states(path, device=True)
    assert pf.last_flagged() == 3
    got = ll.read_states(path, device=True)                    # the count is of the last call
    assert pf.last_flagged() == 3
    assert np.array_equal(pc.bits(got[0]), pc.bits(want[0])) and np.array_equal(got[1], want[1])
    assert want[1][2000] == 3 and want[0][2000] == 12.5 and want[0][51] == 0.0     # a gap
    ragged = _crafted_file(tmp_path, '1H-12C-15N__Ragged.states', ragged=True)
    want, got = ll.read_states(ragged), ll.read_states(ragged, device=True)
    assert np.array_equal(pc.bits(got[0]), pc.bits(want[0])) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match='does not exist'):
        ll.read_states(str(tmp_path / 'none.states'), device=True)


def test_make_tli_with_the_partition_of_exomol_states(tmp_path):
    """Exomol(..., partition=(temps, pf, isotopes)) fed from exomol_states, its states read on
    the device: the TLI's partition block holds those values, its lines are the host route's."""
    g = lc.g32()
    q, isotopes, temps = pf.exomol_states(pc.NH3, 100.0, 3000.0, 100.0)
    kw = dict(isotopes=list(g['nh3_isotopes']), iso_mass=g['nh3_mass'], iso_ratio=g['nh3_ratio'],
              partition=(temps, q, isotopes))
    lo, hi = lc.wn_window(1.9, 2.1)
    dev, host = str(tmp_path / 'dev.tli'), str(tmp_path / 'host.tli')
    ll.make_tli(ll.Exomol([lc.TRANS_14, lc.TRANS_15], device=True, **kw), dev, wn_low=lo,
                wn_high=hi, device=True)
    ll.make_tli(ll.Exomol([lc.TRANS_14, lc.TRANS_15], **kw), host, wn_low=lo, wn_high=hi,
                device=False)
    with open(dev, 'rb') as a, open(host, 'rb') as b:
        assert a.read() == b.read()
    db = tli.read_tli(dev, strict=True)[0][0]
    assert db['isotopes'] == isotopes == ['4111', '5111']
    assert np.array_equal(pc.bits(db['temperatures']), pc.bits(temps))
    assert np.array_equal(pc.bits(db['partition']), pc.bits(q))
