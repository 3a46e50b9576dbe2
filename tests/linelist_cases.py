"""Cases of the line-list tests (test_linelist_cpu.py, test_gpu_linelist.py): the fixture inputs
with the isotope data the reference used for them (g32_linelist.npz), and builders of crafted
records -- a valid HITRAN record with chosen field texts, a valid ExoMol record and states table."""
import atexit
import decimal
import os
import shutil
import struct
import tempfile

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_g32 = None


def g32():
    global _g32
    if _g32 is None:
        with np.load(os.path.join(GOLDEN, 'g32_linelist.npz')) as f:
            _g32 = {k: f[k] for k in f.files}
    return _g32


def _write_inputs():
    """The reference's mock inputs, held in g32 as bytes, as files under their own names (an
    ExoMol file's name carries its molecule, isotope and states file) in a scratch directory
    that lives as long as the process."""
    folder = tempfile.mkdtemp(prefix='pb_linelist_')
    atexit.register(shutil.rmtree, folder, ignore_errors=True)
    for key, raw in g32().items():
        if key.startswith('input_'):
            raw.tofile(os.path.join(folder, key[len('input_'):]))
    return folder


INPUT_DIR = _write_inputs()
PAR = os.path.join(INPUT_DIR, 'Mock_HITRAN_H2O_1.00-1.01um.par')
TRANS_14 = os.path.join(INPUT_DIR, '14N-1H3__MockBYTe__04999-05000.trans')
TRANS_15 = os.path.join(INPUT_DIR, '15N-1H3__MockBYTe-15__04999-05000.trans')
PF_NH3 = os.path.join(INPUT_DIR, 'PF_Exomol_NH3.dat')
INPUTS = dict(h2o=PAR, nh3_14=TRANS_14, nh3_15=TRANS_15)


def h2o_db(ll, files=PAR, partition=None):
    g = g32()
    if partition is None:
        partition = (g['h2o_pf_temp'], g['h2o_pf'], list(g['h2o_pf_isotopes']))
    return ll.Hitran(files, molecule='H2O', isotopes=list(g['h2o_isotopes']),
                     iso_mass=g['h2o_mass'], iso_ratio=g['h2o_ratio'], partition=partition)


def nh3_db(ll, files, partition=PF_NH3):
    g = g32()
    return ll.Exomol(files, isotopes=list(g['nh3_isotopes']), iso_mass=g['nh3_mass'],
                     iso_ratio=g['nh3_ratio'], partition=partition)


def database(ll, key):
    return h2o_db(ll) if key == 'h2o' else nh3_db(ll, INPUTS[key])


# the H2O window of the reference's run (make_golden_e2e.CFG_TLI: 1.00 - 1.01 um) and of the NH3
# run (make_golden_linelist.NH3_WL), as lread.py:130-131 forms them
def wn_window(wl_low_um, wl_high_um):
    return 1.0 / wl_high_um / 1e-4, 1.0 / wl_low_um / 1e-4


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def canonical(wn, gf, elow, iso):
    """The four columns ordered by (isotope, wn, elow, gf): the reference's sort is not stable."""
    order = np.lexsort((gf, elow, wn, iso))
    return wn[order], gf[order], elow[order], np.asarray(iso)[order]


# ---------------------------------------------------------------------------------------------
# crafted records
# ---------------------------------------------------------------------------------------------
def hitran_record(iso='1', wn=' 9901.390499', a21=' 2.318E-04', elow='  920.2098', g2='   21.0',
                  eol=b'\r\n'):
    """One valid 160-character HITRAN record (+ eol) with the given field texts, each exactly as
    wide as its field: wn 12, a21 10, elow 10, g2 7."""
    rec = bytearray(b' ' * 160)
    rec[0:2] = b' 1'
    for text, a, b in ((iso, 2, 3), (wn, 3, 15), (' 4.294E-27', 15, 25), (a21, 25, 35),
                       ('.03270.300', 35, 45), (elow, 45, 55), ('0.51-.015608', 55, 67),
                       (g2, 146, 153), ('   19.0', 153, 160)):
        raw = text.encode('latin-1') if isinstance(text, str) else text
        assert len(raw) == b - a, (text, a, b)
        rec[a:b] = raw
    return bytes(rec) + eol


def exomol_record(up, low, a21, recsize=37):
    """One ExoMol transition record of recsize bytes ending in a line feed: the three tokens
    (texts or numbers) right-justified over the room there is."""
    body = f'{up} {low} {a21}'
    room = recsize - 1
    if len(body) < room:
        wide = (room - 2 - len(str(a21))) // 2
        body = f'{str(up):>{wide}} {str(low):>{wide}} {a21}'
    assert len(body) <= room, (body, recsize)
    return (body.rjust(room) + '\n').encode()


def states_table(rng, nstates, gaps=()):
    """(energy, degeneracy) dense in the id, zero at the ids in `gaps`, energies rising."""
    energy = np.round(np.cumsum(rng.uniform(0.5, 40.0, nstates)), 6)
    degeneracy = rng.integers(1, 200, nstates).astype(np.int64)
    for i in gaps:
        energy[i], degeneracy[i] = 0.0, 0
    return energy, degeneracy


# field texts of the five HITRAN formats and the ExoMol A21 form
def random_field(rng, kind):
    if kind == 'wn':                                           # F12.6
        return f'{rng.uniform(0.0, 99999.0):12.6f}'
    if kind in ('a21', 'a21_fast'):                            # E10.3; _fast: |q| <= 22 only
        lo = -19 if kind == 'a21_fast' else -30
        mantissa = min(rng.uniform(1.0, 10.0), 9.999)
        return f'{mantissa * 10.0 ** int(rng.integers(lo, 9)):10.3E}'
    if kind == 'elow':                                         # F10.4
        return f'{rng.uniform(-1.0, 99999.0):10.4f}'
    if kind == 'g2':                                           # F7.1
        return f'{rng.uniform(0.0, 9999.0):7.1f}'
    if kind == 'digits':                                       # any digits within a width of 12
        n = int(rng.integers(1, 12))
        text = ''.join(rng.choice(list('0123456789'), n))
        p = int(rng.integers(0, n + 1))
        return (text[:p] + '.' + text[p:]).rjust(12)
    assert kind in ('exomol', 'exomol_fast')                   # %.4e; _fast: |q| <= 22 only
    lo = -15 if kind == 'exomol_fast' else -35
    mantissa = min(rng.uniform(1.0, 10.0), 9.9999)
    return f'{mantissa * 10.0 ** int(rng.integers(lo, 12)):.4e}'


FAST_TEXTS = ['-.015608', '.5', '5.', '  5.25  ', '0.000E+00', '-0.0', '+1.5e+3', '1E22',
              '9007199254740992', '12345678.9012']
# outside the fast path: more digits, larger exponents, and what is not in the grammar
FLAGGED_TEXTS = ['1.000E-38', '9.999E+30', '12345678901234567890', '9007199254740993', 'nan',
                 '1_0', '', '1.2.3']


def fast_path_rule(text):
    """Is the field inside w <= 2^53, |q| <= 22?  From decimal's reading of the text, which is
    independent of the code under test; texts outside the decimal grammar are outside."""
    try:
        sign, digits, exponent = decimal.Decimal(text.strip(' ')).as_tuple()
    except decimal.InvalidOperation:
        return False
    if not isinstance(exponent, int) or '_' in text:
        return False
    w = int(''.join(map(str, digits)))
    return w <= 2**53 and abs(exponent) <= 22


def same_bits(a, b):
    return struct.pack('d', a) == struct.pack('d', b)


def same_columns(got, want):
    """Equal bit for bit, NaN where the other side has NaN (a NaN's payload is not compared)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(bits(got[~nan]), bits(want[~nan]))
