"""Line lists to TLI, host route (pyratbay_amd/linelist.py with device=False) against what the
reference's readers returned for its mock inputs (g32_linelist.npz) and the TLI files it wrote."""
import ctypes as C
import os

import numpy as np
import pytest

import linelist_cases as lc
from pyratbay_amd import linelist as ll
from pyratbay_amd import tli

G = lc.g32()
KEYS = ('h2o', 'nh3_14', 'nh3_15')


def _window_read(key, a, b):
    db = lc.database(ll, key)
    file = db.files[0]
    win = file.window(db, a, b)
    return db, file, win


@pytest.mark.parametrize('key', KEYS)
def test_host_parse_equals_reference_for_every_window(key):
    """Record size, record count, istart / istop and the four arrays of dbread, bit for bit, for
    every window of make_golden_tli.windows(); no record of the fixtures is off the fast path."""
    db = lc.database(ll, key)
    file = db.files[0]
    assert (file.recsize, file.nrec) == (int(G[f'{key}_recsize']), int(G[f'{key}_nrec']))
    for k, (a, b) in enumerate(G[f'{key}_windows']):
        win = file.window(db, a, b)
        if G[f'{key}_w{k}_none']:
            assert win is None
            continue
        assert win == (int(G[f'{key}_w{k}_istart']), int(G[f'{key}_w{k}_istop'])), (k, a, b)
        wn, gf, elow, iso = ll._read_host(db, file, *win)
        for name, got in (('wn', wn), ('gf', gf), ('elow', elow)):
            assert np.array_equal(lc.bits(got), lc.bits(G[f'{key}_w{k}_{name}'])), (k, name)
        assert np.array_equal(iso, G[f'{key}_w{k}_iso'])


@pytest.mark.parametrize('key', KEYS)
def test_no_fixture_record_is_flagged(key):
    """The condition the device tests rest on: every numeric field of the fixture inputs is on
    the fast path (A21 mantissas of 4 digits with exponents -6 ... 0, everything else fixed-point
    with at most 12 digits)."""
    db = lc.database(ll, key)
    file = db.files[0]
    with open(file.path, 'rb') as f:
        data = f.read(file.nrec * file.recsize)
    for i in range(file.nrec):
        rec = data[i * file.recsize:(i + 1) * file.recsize]
        if key == 'h2o':
            fields = [rec[a:b] for _, a, b in ll.HITRAN_FIELDS]
            assert rec[2:3].decode() in ll.HITRAN_ISO
        else:
            fields = [rec.split()[2]]
            assert all(t.isdigit() and len(t) <= 18 for t in rec.split()[:2])
        for text in fields:
            value, flagged = ll.decimal_fast_path_host(text)
            assert not flagged and lc.same_bits(value, float(text)), (i, text)


def test_decimal_fast_path_equals_float():
    """20 000 seeded random field texts of the five HITRAN formats and the ExoMol %.4e form: the
    bits of float(), and flagged exactly outside w <= 2^53, |q| <= 22 (judged from decimal's
    reading of the text); then the crafted texts."""
    rng = np.random.default_rng(32)
    kinds = ('wn', 'a21', 'elow', 'g2', 'digits', 'exomol')
    nflag = 0
    for i in range(20000):
        text = lc.random_field(rng, kinds[i % len(kinds)])
        value, flagged = ll.decimal_fast_path_host(text)
        assert flagged == (not lc.fast_path_rule(text)), text
        nflag += flagged
        if not flagged:
            assert lc.same_bits(value, float(text)), text
    assert 0 < nflag < 20000                                   # both routes were met
    for text in lc.FAST_TEXTS:
        value, flagged = ll.decimal_fast_path_host(text)
        assert not flagged and lc.same_bits(value, float(text)), text
    assert lc.same_bits(ll.decimal_fast_path_host('-0.0')[0], -0.0)
    for text in lc.FLAGGED_TEXTS:
        value, flagged = ll.decimal_fast_path_host(text)
        assert flagged and np.isnan(value), text
        assert not lc.fast_path_rule(text), text


def test_binsearch_host_at_equal_values_and_ends():
    values = [1.0, 2.0, 2.0, 2.0, 3.0, 5.0, 5.0, 7.0]
    def wave(i):
        return values[i]
    n = len(values) - 1
    # worked by hand from driver.py:103-132: the bisection ends at lo = 3 (the last 2.0), hi = 4;
    # the walk down starts at hi and moves only over records ABOVE the target, so it stays
    assert ll.binsearch_host(wave, 2.0, 0, n, searchup=False) == 4
    assert ll.binsearch_host(wave, 2.0, 0, n, searchup=True) == 3
    assert ll.binsearch_host(wave, 4.0, 0, n, searchup=False) == 5
    assert ll.binsearch_host(wave, 4.0, 0, n, searchup=True) == 4
    assert ll.binsearch_host(wave, 0.0, 0, n, searchup=False) == 0
    assert ll.binsearch_host(wave, 9.0, 0, n, searchup=True) == n
    assert ll.binsearch_host(wave, 5.0, 5, n, searchup=True) == 6


def _columns_of(path):
    dbs, wn, gf, elow, iso_id, meta = tli.read_tli(path, strict=True)
    return dbs, lc.canonical(wn, gf, elow, meta['iso_global']), meta


def _assert_same_tli(ours, theirs):
    with open(ours, 'rb') as f, open(theirs, 'rb') as g:
        a, b = f.read(), g.read()
    assert len(a) == len(b)
    nlines = tli.read_tli(theirs, strict=True)[5]['n_lines']
    header = len(b) - 26 * nlines
    assert a[:header] == b[:header]                            # the header, byte for byte
    (_, cols_a, meta_a), (_, cols_b, meta_b) = _columns_of(ours), _columns_of(theirs)
    assert np.array_equal(meta_a['lines_per_isotope'], meta_b['lines_per_isotope'])
    for x, y in zip(cols_a[:3], cols_b[:3]):
        assert np.array_equal(lc.bits(x), lc.bits(y))
    assert np.array_equal(cols_a[3], cols_b[3])


def test_make_tli_h2o_equals_reference_file(tmp_path):
    out = str(tmp_path / 'h2o.tli')
    lo, hi = lc.wn_window(1.00, 1.01)
    dbs = ll.make_tli([lc.h2o_db(ll)], out, wn_low=lo, wn_high=hi, device=False)
    assert [d['name'] for d in dbs] == ['HITRAN H2O'] and len(dbs[0]['wn']) == 888
    _assert_same_tli(out, os.path.join(lc.GOLDEN, 'g13_mock_h2o.tli'))


def test_make_tli_nh3_two_files_one_database(tmp_path):
    theirs = str(tmp_path / 'reference.tli')
    G['nh3_tli'].tofile(theirs)
    out = str(tmp_path / 'nh3.tli')
    lo, hi = lc.wn_window(*G['nh3_tli_wl'])
    dbs = ll.make_tli([lc.nh3_db(ll, lc.TRANS_14), lc.nh3_db(ll, lc.TRANS_15)], out,
                      wn_low=lo, wn_high=hi, device=False)
    assert len(dbs) == 1 and dbs[0]['name'] == 'Exomol NH3'
    assert list(dbs[0]['isotopes']) == ['4111', '5111']
    _assert_same_tli(out, theirs)
    # one object with both files is the same database
    both = str(tmp_path / 'both.tli')
    ll.make_tli(lc.nh3_db(ll, [lc.TRANS_14, lc.TRANS_15]), both, wn_low=lo, wn_high=hi,
                device=False)
    with open(out, 'rb') as f, open(both, 'rb') as g:
        assert f.read() == g.read()


def test_par_split_in_two_files(tmp_path):
    """The .par split at record 400 gives the file of the whole one, by wavelengths too."""
    with open(lc.PAR, 'rb') as f:
        data = f.read()
    parts = []
    for name, chunk in (('a.par', data[:400 * 162]), ('b.par', data[400 * 162:])):
        parts.append(str(tmp_path / name))
        with open(parts[-1], 'wb') as f:
            f.write(chunk)
    lo, hi = lc.wn_window(1.00, 1.01)
    whole, split = str(tmp_path / 'whole.tli'), str(tmp_path / 'split.tli')
    ll.make_tli(lc.h2o_db(ll), whole, wn_low=lo, wn_high=hi, device=False)
    ll.make_tli(lc.h2o_db(ll, parts), split, wl_low=1.0 / hi, wl_high=1.0 / lo, device=False)
    a, b = tli.read_tli(whole, strict=True), tli.read_tli(split, strict=True)
    for x, y in zip(a[1:5], b[1:5]):
        assert np.array_equal(x, y)


def _write(path, records):
    with open(path, 'wb') as f:
        f.write(b''.join(records))
    return str(path)


def test_refusals(tmp_path):
    lo, hi = 9000.0, 11000.0
    out = str(tmp_path / 'x.tli')
    good = [lc.hitran_record(wn=f'{9900.0 + i:12.6f}') for i in range(6)]

    # elow <= 0 is dropped, not refused
    recs = list(good)
    recs[2] = lc.hitran_record(wn=f'{9902.0:12.6f}', elow='   -1.0000')
    recs[3] = lc.hitran_record(wn=f'{9903.0:12.6f}', elow='    0.0000')
    dbs = ll.make_tli(lc.h2o_db(ll, _write(tmp_path / 'drop.par', recs)), out, wn_low=lo,
                      wn_high=hi, device=False)
    assert list(dbs[0]['wn']) == [9900.0, 9901.0, 9904.0, 9905.0]

    recs = list(good)
    recs[4] = lc.hitran_record(iso='C', wn=f'{9904.0:12.6f}')
    path = _write(tmp_path / 'iso.par', recs)
    with pytest.raises(ValueError, match=r'iso\.par: record 4: field iso'):
        ll.make_tli(lc.h2o_db(ll, path), out, wn_low=lo, wn_high=hi, device=False)

    recs = list(good)
    recs[3] = lc.hitran_record(wn=f'{9903.0:12.6f}', a21=' 2.3x8E-04')
    path = _write(tmp_path / 'a21.par', recs)
    with pytest.raises(ValueError, match=r'a21\.par: record 3: field a21: could not convert'):
        ll.make_tli(lc.h2o_db(ll, path), out, wn_low=lo, wn_high=hi, device=False)

    # a state id equal to the number of states
    rng = np.random.default_rng(5)
    energy, degeneracy = lc.states_table(rng, 40)
    with open(tmp_path / '14N-1H3__Crafted.states', 'w') as f:
        for i in range(40):
            f.write(f'{i:12d} {energy[i]:12.6f} {degeneracy[i]:6d}\n')
    recs = [lc.exomol_record(30 + i, i, '1.0000e-03') for i in range(8)]
    recs[5] = lc.exomol_record(40, 5, '1.0000e-03')
    path = _write(tmp_path / '14N-1H3__Crafted__0-1.trans', recs)
    with pytest.raises(ValueError, match=r'0-1\.trans: record 5: field up: state id 40'):
        ll.make_tli(lc.nh3_db(ll, path), out, wn_low=-np.inf, wn_high=np.inf, device=False)

    for kind in ('tips', 'poly'):
        with pytest.raises(ValueError, match='not shipped'):
            lc.h2o_db(ll, partition=kind)

    with pytest.raises(ValueError, match='none of its files overlaps'):
        ll.make_tli(lc.h2o_db(ll), out, wn_low=100.0, wn_high=200.0, device=False)

    # an isotope with lines and no partition function: the reference's message
    g = lc.g32()
    short = (g['h2o_pf_temp'], g['h2o_pf'][:1], list(g['h2o_pf_isotopes'][:1]))
    with pytest.raises(ValueError, match='No partition functions found for these isotopes of '
                                         'the H2O line list'):
        ll.make_tli(lc.h2o_db(ll, partition=short), out, wn_low=lo, wn_high=hi, device=False)
    with pytest.raises(ValueError, match='No partition functions found'):
        ll.make_tli(lc.nh3_db(ll, lc.TRANS_15, partition=([1.0, 2.0], [[1.0, 2.0]], ['4111'])),
                    out, wn_low=-np.inf, wn_high=np.inf, device=False)


def test_helpers_read_the_callers_files(tmp_path):
    assert ll.get_exomol_mol('1H2-16O__POKAZATEL__00400-00500.trans.bz2') == ('H2O', '116')
    assert ll.get_exomol_mol('12C-16O2__HITEMP.pf') == ('CO2', '266')
    assert ll.get_exomol_mol('12C-1H3-2H__MockName__01100-01200.trans.bz2') == ('CH4', '21112')
    assert ll.exomol_states_file(lc.TRANS_14).endswith('14N-1H3__MockBYTe.states')
    pf, iso, temp = ll.read_pf(lc.PF_NH3)
    assert iso == ['4111', '5111'] and pf.shape == (2, len(temp)) and temp[0] == 1.0
    assert pf[0, 0] == 3.8341 and pf[1, 1] == 4.6386
    path = tmp_path / 'isotopes.dat'
    path.write_text('# comment\n\nH2O   161  116   0.997317300   18.010560\n'
                    'NH3  5111  5111  0.003661289   18.023580\n')
    mol, hit, exo, ratio, mass = ll.read_isotopes(str(path))
    assert list(mol) == ['H2O', 'NH3'] and list(exo) == ['116', '5111']
    assert ratio[1] == 0.003661289 and mass[0] == 18.010560


def test_entry_points_check_arguments_before_hip():
    """Every new entry point refuses bad arguments before any HIP call, GPU or not (the pointers
    are never dereferenced: a good call with no records returns at once)."""
    from pyratbay_amd import _capi
    lib = _capi.lib()
    for name in ('pb_parse_hitran', 'pb_parse_exomol', 'pb_linelist_gf'):
        assert name in _capi.exported_names()
    p = 4096

    def hitran(text=p, nrec=0, recsize=162, out=p):
        return lib.pb_parse_hitran(text, nrec, recsize, p, p, p, out, p, p, p, None)

    def exomol(text=p, nrec=0, recsize=37, nstates=10, iso=0, out=p):
        return lib.pb_parse_exomol(text, nrec, recsize, p, p, nstates, iso, p, p, p, out, p, p,
                                   p, None)

    def refused(rc, text):
        assert rc == _capi.constant('PB_ERR_ARG'), (text, rc)
        assert text in lib.pb_last_error().decode(), lib.pb_last_error()
    assert hitran() == 0 and exomol() == 0
    assert lib.pb_linelist_gf(p, p, p, 0, 1.0, 1.0, p, None) == 0
    refused(hitran(text=None), 'pb_parse_hitran: null pointer')
    refused(hitran(out=None), 'pb_parse_hitran: null pointer')
    refused(hitran(nrec=-1), '-1 records')
    refused(hitran(nrec=2**31), 'records')
    refused(hitran(recsize=152), 'records of 152 bytes')
    refused(hitran(recsize=256), 'records of 256 bytes')
    refused(exomol(text=None), 'pb_parse_exomol: null pointer')
    refused(exomol(nrec=-1), '-1 records')
    refused(exomol(recsize=4), 'records of 4 bytes')
    refused(exomol(nstates=0), '0 states')
    refused(exomol(iso=32768), 'isotope index 32768')
    refused(lib.pb_linelist_gf(p, p, p, -1, 1.0, 1.0, p, None), '-1 lines')
    refused(lib.pb_linelist_gf(p, None, p, 0, 1.0, 1.0, p, None), 'pb_linelist_gf: null pointer')
    assert (_capi.constant('PB_LL_HITRAN_G2'), _capi.constant('PB_LL_EXOMOL_STATE')) == (16, 16)
    assert {k: _capi.constant('PB_LL_HITRAN_' + k.upper()) for k in ll.HITRAN_FLAGS} == \
        ll.HITRAN_FLAGS
    assert {k: _capi.constant('PB_LL_EXOMOL_' + k.upper()) for k in ll.EXOMOL_FLAGS} == \
        ll.EXOMOL_FLAGS
    assert C.sizeof(C.c_int16) == 2
