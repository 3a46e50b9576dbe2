"""Line lists to TLI on the device (pb_parse_hitran, pb_parse_exomol, pb_linelist_gf and
make_tli(device=True)) against the host route of pyratbay_amd/linelist.py, bit for bit."""
import os

import numpy as np
import pytest

import linelist_cases as lc
from pyratbay_amd import linelist as ll

pytestmark = pytest.mark.gpu
COLUMNS = ('wn', 'elow', 'a21', 'g2')
GUARD = 64                                     # elements in front of and behind every output


class Parsed:
    pass


def _parse(kind, data, nrec, recsize, offset=0, states=None, iso=0):
    """One launch of a parse kernel at the kernel boundary: text_d `offset` bytes behind a 16-byte
    boundary, every output inside a larger buffer filled with NaN / 0x7f whose guard elements
    must come back untouched; then pb_linelist_gf on the columns."""
    import torch
    from pyratbay_amd._capi import call
    from pyratbay_amd._device import _ptr, _stream
    raw = np.frombuffer(bytes(data[:nrec * recsize]), np.uint8)
    text = torch.full((offset + len(raw) + 16,), 0x7f, dtype=torch.uint8, device='cuda')
    assert text.data_ptr() % 16 == 0
    text[offset:offset + len(raw)] = torch.from_numpy(raw.copy()).cuda()
    buf = {c: torch.full((nrec + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
           for c in COLUMNS + ('gf',)}
    buf['iso'] = torch.full((nrec + 2 * GUARD,), 0x7f7f, dtype=torch.int16, device='cuda')
    buf['flags'] = torch.full((nrec + 2 * GUARD,), 0x7f, dtype=torch.uint8, device='cuda')
    count = torch.zeros(3, dtype=torch.int32, device='cuda')
    out = {c: b[GUARD:GUARD + nrec] for c, b in buf.items()}
    args = [_ptr(out[c]) for c in COLUMNS + ('iso', 'flags')] + [_ptr(count[1:2]), _stream()]
    if kind == 'hitran':
        call('pb_parse_hitran', _ptr(text[offset:]), nrec, recsize, *args)
    else:
        energy, degeneracy = states
        e_d = torch.from_numpy(np.asarray(energy, np.float64)).cuda()
        g_d = torch.from_numpy(np.asarray(degeneracy, np.float64)).cuda()
        call('pb_parse_exomol', _ptr(text[offset:]), nrec, recsize, _ptr(e_d), _ptr(g_d),
             len(energy), iso, *args)
    call('pb_linelist_gf', _ptr(out['wn']), _ptr(out['a21']), _ptr(out['g2']), nrec, ll.C1,
         ll.GF_DIVISOR, _ptr(out['gf']), _stream())
    torch.cuda.synchronize()
    r = Parsed()
    for c, b in buf.items():
        host = b.cpu().numpy()
        guard = np.concatenate([host[:GUARD], host[GUARD + nrec:]])
        if host.dtype == np.float64:
            assert np.all(np.isnan(guard)), c
        else:
            assert np.all(guard == (0x7f7f if c == 'iso' else 0x7f)), c
        setattr(r, c, host[GUARD:GUARD + nrec].copy())
    counts = count.cpu().numpy()
    assert counts[0] == 0 and counts[2] == 0
    r.count = int(counts[1])
    return r


def _fixture(key):
    db = lc.database(ll, key)
    file = db.files[0]
    with open(file.path, 'rb') as f:
        data = f.read(file.nrec * file.recsize)
    if key == 'h2o':
        host = ll.parse_hitran_host(data, file.recsize)
        return 'hitran', data, file, None, host
    host = ll.parse_exomol_host(data, file.recsize, file.energy, file.degeneracy)
    host = host + (np.full(file.nrec, file.iso, np.int16),)
    return 'exomol', data, file, (file.energy, file.degeneracy), host


def _assert_equal_host(r, host, n):
    wn, elow, a21, g2, iso = (h[:n] for h in host)
    for name, want in (('wn', wn), ('elow', elow), ('a21', a21), ('g2', g2),
                       ('gf', ll.gf_host(wn, a21, g2))):
        assert np.array_equal(lc.bits(getattr(r, name)), lc.bits(want)), (name, n)
    assert np.array_equal(r.iso, iso)
    assert not r.flags.any() and r.count == 0


@pytest.mark.parametrize('key', ['h2o', 'nh3_14', 'nh3_15'])
def test_columns_equal_host_route(key):
    """One lane, one wavefront, one workgroup, each with one record more and one fewer, and the
    whole file; text at byte offsets 0, 1, 7, 15 from a 16-byte boundary; guards untouched."""
    kind, data, file, states, host = _fixture(key)
    iso = getattr(file, 'iso', 0)
    for n in (1, 63, 64, 65, 255, 256, 257, file.nrec):
        for offset in (0, 1, 7, 15):
            r = _parse(kind, data, n, file.recsize, offset, states, iso)
            _assert_equal_host(r, host, n)


def test_record_sizes_162_and_161():
    """The same records with CR LF and with LF only."""
    kind, data, file, _, host = _fixture('h2o')
    assert file.recsize == 162 and data[160:162] == b'\r\n'
    lf = data.replace(b'\r\n', b'\n')
    assert len(lf) == 161 * file.nrec
    for offset in (0, 7):
        _assert_equal_host(_parse(kind, lf, file.nrec, 161, offset), host, file.nrec)


def _crafted_hitran(rng, n):
    records = []
    for i in range(n):
        records.append(lc.hitran_record(
            iso='1234567890AB'[int(rng.integers(0, 12))], wn=lc.random_field(rng, 'wn'),
            a21=lc.random_field(rng, 'a21_fast'), elow=lc.random_field(rng, 'elow'),
            g2=lc.random_field(rng, 'g2')))
    return records


# (field, text of the field's width) that float() reads and the device must leave to the host
WIDTH = {name: b - a for name, a, b in ll.HITRAN_FIELDS}
FLAGGED_FORMS = [(field, text.rjust(WIDTH[field])) for field, text in (
    ('a21', '1.000E-38'), ('a21', '9.999E+30'), ('a21', 'nan'), ('a21', '1_0.5'),
    ('wn', '1_000.000000'), ('wn', 'inf'), ('elow', '1.0000E-30'), ('g2', '1_0.0'))]


def test_crafted_records_and_the_flagged_route(tmp_path):
    """4096 crafted records with seeded random digits in every field equal float() per field; 64
    of them, in 64 different wavefronts, carry forms outside the fast path: the counter reads
    64, the flag bits name the fields, and the chunk loop's patch gives the host route's
    columns and gf."""
    import torch
    rng = np.random.default_rng(3232)
    n = 4096
    records = _crafted_hitran(rng, n)
    want_flags = np.zeros(n, np.uint8)
    for k in range(64):
        i = 64 * k + (7 * k) % 64
        field, text = FLAGGED_FORMS[k % len(FLAGGED_FORMS)]
        records[i] = lc.hitran_record(**{'wn': f'{9000.0 + k:12.6f}', field: text})
        want_flags[i] = ll.HITRAN_FLAGS[field]
    data = b''.join(records)
    host = ll.parse_hitran_host(data, 162)
    for name, a, b in ll.HITRAN_FIELDS:                       # the host route is float() itself
        col = host[COLUMNS.index(name)]
        for i in (0, 1, 2049, n - 1):
            assert lc.same_bits(col[i], float(records[i][a:b]))
    r = _parse('hitran', data, n, 162, offset=7)
    assert r.count == 64 and np.array_equal(r.flags, want_flags)
    clean = want_flags == 0
    for name, want in zip(COLUMNS, host):
        assert np.array_equal(lc.bits(getattr(r, name)[clean]), lc.bits(want[clean])), name
        flagged_here = want_flags == ll.HITRAN_FLAGS[name]
        assert np.all(np.isnan(getattr(r, name)[flagged_here])), name
    assert np.array_equal(r.iso, host[4])

    # the chunk loop: flagged records patched from the pinned bytes, then gf for every record
    path = str(tmp_path / 'crafted.par')
    with open(path, 'wb') as f:
        f.write(data)
    db = lc.h2o_db(ll, path)
    chunker = ll._Chunker(1000 * 162 + 5)
    ll._last_flagged = 0
    wn, gf, elow, iso = (t.cpu().numpy() for t in
                         ll._read_device(db, db.files[0], 0, n - 1, chunker))
    assert ll.last_flagged() == 64 and chunker.used == [3, 2]
    good = host[1] > 0
    h_wn, h_elow, h_a21, h_g2, h_iso = (h[good] for h in host)
    with np.errstate(over='ignore'):
        want_gf = ll.gf_host(h_wn, h_a21, h_g2)
    for got, want in ((wn, h_wn), (elow, h_elow), (gf, want_gf)):
        assert lc.same_columns(got, want)
    assert np.isnan(want_gf).any() and np.isinf(h_wn).any()     # the nan and the inf got there
    assert np.array_equal(iso, h_iso)
    torch.cuda.synchronize()

    # a field that Python refuses too: the file, the record and the field
    records[777] = lc.hitran_record(elow=' ' * 10)
    with open(path, 'wb') as f:
        f.write(b''.join(records))
    db = lc.h2o_db(ll, path)
    with pytest.raises(ValueError, match=r'crafted\.par: record 777: field elow: could not'):
        ll._read_device(db, db.files[0], 0, n - 1, chunker)
    torch.cuda.synchronize()


def test_exomol_cases(tmp_path):
    rng = np.random.default_rng(77)
    nstates = 300
    energy, degeneracy = lc.states_table(rng, nstates, gaps=(0, 17, 100, 299))
    up = rng.integers(1, nstates, 200)
    low = rng.integers(1, nstates, 200)
    up[5] = low[5] = 42                                        # wn = 0: gf is the IEEE result
    up[6], low[6] = 17, 100                                    # both in gaps
    a21 = [lc.random_field(rng, 'exomol_fast') for _ in range(200)]
    a21[9] = '12345678901234567890e-19'                        # a 20-digit mantissa: the host's
    for recsize in (37, 38):
        records = [lc.exomol_record(u, l, a, recsize) for u, l, a in zip(up, low, a21)]
        data = b''.join(records)
        host = ll.parse_exomol_host(data, recsize, energy, degeneracy)
        r = _parse('exomol', data, 200, recsize, offset=1, states=(energy, degeneracy), iso=1)
        want_flags = np.zeros(200, np.uint8)
        want_flags[9] = ll.EXOMOL_FLAGS['a21']
        assert r.count == 1 and np.array_equal(r.flags, want_flags)
        ok = want_flags == 0
        for name, want in zip(COLUMNS, host):
            assert np.array_equal(lc.bits(getattr(r, name)[ok]), lc.bits(want[ok])), name
        with np.errstate(divide='ignore', invalid='ignore'):
            want_gf = ll.gf_host(*(host[j] for j in (0, 2, 3)))
        assert lc.same_columns(r.gf[ok], want_gf[ok]) and np.isnan(want_gf[6])
        assert r.wn[5] == 0.0 and np.isinf(r.gf[5]) and np.all(r.iso == 1)

    # tokens of the smallest and the largest widths the record size allows
    small = b''.join(f'{u} {l} {a}\n'.encode() for u, l, a in ((1, 2, 3), (9, 8, 7), (5, 5, 1)))
    r = _parse('exomol', small, 3, 6, offset=15, states=(energy, degeneracy))
    host = ll.parse_exomol_host(small, 6, energy, degeneracy)
    assert r.count == 0
    for name, want in zip(COLUMNS, host):
        assert np.array_equal(lc.bits(getattr(r, name)), lc.bits(want)), name
    wide = [f'{u:018d} {l:018d} {1.25e-3 * (k + 1):.214f}\n'
            for k, (u, l) in enumerate(((1, 2), (298, 3), (150, 151)))]
    wide = ''.join(wide).encode()
    assert len(wide) == 3 * 255
    r = _parse('exomol', wide, 3, 255, offset=7, states=(energy, degeneracy))
    host = ll.parse_exomol_host(wide, 255, energy, degeneracy)
    assert r.count == 3 and np.all(r.flags == ll.EXOMOL_FLAGS['a21'])   # 200 digits: the host's
    for name in ('wn', 'elow', 'g2'):
        assert np.array_equal(lc.bits(getattr(r, name)), lc.bits(host[COLUMNS.index(name)]))

    # a missing token and an id equal to nstates: flag bits of their own, nothing is loaded
    records = [lc.exomol_record(u, l, a) for u, l, a in zip(up[:70], low[:70], a21[:70])]
    records[9] = lc.exomol_record(up[9], low[9], '1.0000e-03')
    records[3] = ('230'.rjust(12).ljust(36) + '\n').encode()
    records[66] = lc.exomol_record(nstates, 7, '1.0000e-03')
    r = _parse('exomol', b''.join(records), 70, 37, states=(energy, degeneracy))
    assert r.count == 2 and r.flags[3] == ll.EXOMOL_FLAGS['token']
    assert r.flags[66] == ll.EXOMOL_FLAGS['state'] and np.count_nonzero(r.flags) == 2
    assert np.isnan(r.wn[66]) and np.isnan(r.wn[3])
    # through make_tli the state id is refused with the file, the record and the field
    with open(tmp_path / '14N-1H3__Crafted.states', 'w') as f:
        for i in range(nstates):
            f.write(f'{i:12d} {energy[i]:12.6f} {degeneracy[i]:6d}\n')
    records[3] = lc.exomol_record(up[3], low[3], '1.0000e-03')
    path = str(tmp_path / '14N-1H3__Crafted__0-1.trans')
    with open(path, 'wb') as f:
        f.write(b''.join(records))
    db = lc.nh3_db(ll, path)
    with pytest.raises(ValueError, match=r'0-1\.trans: record 66: field up: state id 300'):
        ll._read_device(db, db.files[0], 0, 69, ll._Chunker(1 << 16))


def _dbs(which):
    h2o = [lc.h2o_db(ll)]
    nh3 = [lc.nh3_db(ll, lc.TRANS_14), lc.nh3_db(ll, lc.TRANS_15)]
    return {'h2o': h2o, 'nh3': nh3, 'both': h2o + nh3}[which]


@pytest.mark.parametrize('which', ['h2o', 'nh3', 'both'])
def test_make_tli_device_writes_the_host_routes_bytes(tmp_path, which):
    """Both sorts are stable: the same bytes, for one chunk, for chunks of ten records and seven
    bytes, and for chunks of 257 records (whole records per chunk, both buffers and streams
    used, a partial last chunk)."""
    host, dev = str(tmp_path / 'host.tli'), str(tmp_path / 'dev.tli')
    lo, hi = (0.0, 20000.0) if which == 'both' else \
        lc.wn_window(1.00, 1.01) if which == 'h2o' else lc.wn_window(1.9, 2.1)
    ll.make_tli(_dbs(which), host, wn_low=lo, wn_high=hi, device=False)
    with open(host, 'rb') as f:
        want = f.read()
    recsize = 162 if which != 'nh3' else 38
    for chunk_bytes, both_buffers in ((1 << 20, False), (10 * recsize + 7, True),
                                      (257 * recsize, True)):
        out = ll.make_tli(_dbs(which), dev, wn_low=lo, wn_high=hi, device=True,
                          chunk_bytes=chunk_bytes)
        with open(dev, 'rb') as f:
            assert f.read() == want, chunk_bytes
        assert ll.last_flagged() == 0
        assert all(isinstance(d['wn'], np.ndarray) for d in out)
        if both_buffers:
            assert min(ll.last_chunks()) >= 1
    if which == 'both':
        assert [d['name'] for d in out] == ['HITRAN H2O', 'Exomol NH3']


def test_make_tli_refuses_before_any_launch(tmp_path, monkeypatch):
    out = str(tmp_path / 'x.tli')
    with pytest.raises(ValueError, match='none of its files overlaps'):
        ll.make_tli(lc.h2o_db(ll), out, wn_low=100.0, wn_high=200.0, device=True)
    # columns and sort scratch that do not fit: 888 lines at a terabyte each
    monkeypatch.setattr(ll, '_DEVICE_BYTES_PER_LINE', 1 << 40)
    with pytest.raises(ValueError, match='of device memory'):
        ll.make_tli(lc.h2o_db(ll), out, wn_low=0.0, wn_high=20000.0, device=True)
    assert not os.path.exists(out)


def test_spectrum_from_the_written_file(golden, tmp_path):
    """LBLSpectrum.from_tli on the written H2O file against the one on the reference's file:
    rtol 1e-12 (the order of tied lines may change a co-added sum's last bits)."""
    from pyratbay_amd import engine
    out = str(tmp_path / 'h2o.tli')
    lo, hi = lc.wn_window(1.00, 1.01)
    ll.make_tli(lc.h2o_db(ll), out, wn_low=lo, wn_high=hi, device=True)
    g = golden('g6_e2e_transit')
    grid = dict(wn=g['wn'], own=g['own'], ownstep=float(g['ownstep']), onwave=int(g['onwave']),
                nwave=len(g['wn']), wnosamp=int(g['wnosamp']), divisors=g['divisors'],
                wnstep=float(g['wn'][1] - g['wn'][0]))
    species = [f'X{i}' for i in range(len(g['mol_mass']))]
    species[int(g['iso_atm_index'][0])] = 'H2O'
    atm = dict(temp=g['temp'], dens=g['dens'], radius=g['radius'], press=g['press'],
               species=species, mol_mass=g['mol_mass'], mol_radius=g['mol_radius'],
               rstar=float(g['rstar']))
    kw = dict(ethresh=float(g['ethresh']), maxdepth=float(g['maxdepth']), rt_path='transit',
              itop=int(g['rtop']), extent=float(g['extent']), cutoff=float(g['cutoff']),
              dlratio=float(g['dlratio']), lorentz=g['lorentz'], doppler=g['doppler'])
    spectra = []
    for path in (out, os.path.join(lc.GOLDEN, 'g13_mock_h2o.tli')):
        m = engine.LBLSpectrum.from_tli(path, atm, grid, **kw)
        spectra.append(m.run().cpu().numpy().copy())
    assert np.all(spectra[1] > 0)
    np.testing.assert_allclose(spectra[0], spectra[1], rtol=1e-12)
