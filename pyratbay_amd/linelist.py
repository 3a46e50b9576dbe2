"""Line lists to a TLI file: the reference's `runmode = tli` for HITRAN/HITEMP `.par` files and
ExoMol `.trans` / `.states` pairs (pyratbay/opacity/lread.py:make_tli,
opacity/linelist/{driver,hitran,exomol}.py).

    from pyratbay_amd import linelist as ll
    h2o = ll.Hitran(files, molecule='H2O', isotopes=[...], iso_mass=[...], iso_ratio=[...],
                    partition=(temps, pf, pf_isotopes))        # or partition='PF_file.dat'
    nh3 = ll.Exomol(trans_files, isotopes=[...], iso_mass=[...], iso_ratio=[...], partition=...)
    dbs = ll.make_tli([h2o, nh3], 'out.tli', wn_low=..., wn_high=...)

The reference reads a record per turn of a Python loop: one seek, one read, five float() calls.
Here the bytes of the window's records go to the device in chunks and one lane parses one record
(csrc/pb_linelist.hip: pb_parse_hitran, pb_parse_exomol, pb_linelist_gf); the elow filter, the
concatenation of a database's files and the stable sort by (isotope, wavenumber, input order) run
on the device tensors.  `device=False` is the host route: the same results stated record by record
with float() and int() on slices, as the reference does.  It needs no GPU.

Text to double: the device takes a field only when it is on the exact fast path of the conversion
(decimal_fast_path_host is the kernel's rule in Python).  Every other field is flagged; after each
chunk the host parses the flagged fields with float() / int() from the bytes it still holds and
patches the columns, or raises ValueError naming the file, the record and the field where Python
itself refuses.  last_flagged() reports how many records took that route in the last make_tli.

The isotope names, masses and ratios come from the caller (read_isotopes() reads a file in the
layout of the reference's isotopes.dat, read_pf() its tabulated partition functions): the
reference's data files are not shipped.

Out of scope: the reference's other readers (pands, tioschwenke, vald, voplez, repack); TIPS and
polynomial partition functions (partition='tips' / 'poly' are refused; partitions.py makes a
tabulated partition from ExoMol states, ExoMol `.pf` files or Kurucz files instead); a correctly
rounded device conversion beyond the fast path (the flagged route covers it); compressed
`.trans.bz2` transitions (`.states.bz2` is read).
"""
import bz2
import itertools
import math
import os
import re

import numpy as np

from . import tli as _tli

# the reference's constants (constants/astrophysical_constants.py:69,110,126,129): scipy.constants'
# m_e * 1e3 and c * 1e2 (CODATA 2022), e in statcoulombs as it writes it
_ME = 9.1093837139e-31 * 1e3
_C = 299792458.0 * 1e2
_E = 4.803205e-10
C1 = _ME * _C**2 / (_E**2 * math.pi)
GF_DIVISOR = 8.0 * np.pi * _C

HITRAN_FIELDS = (('wn', 3, 15), ('a21', 25, 35), ('elow', 45, 55), ('g2', 146, 153))
HITRAN_END = 153
HITRAN_ISO = {c: i for i, c in enumerate('1234567890AB')}
# flag bits of a record (include/pbhip.h, PB_LL_*)
HITRAN_FLAGS = dict(iso=1, wn=2, a21=4, elow=8, g2=16)
EXOMOL_FLAGS = dict(up=1, low=2, a21=4, token=8, state=16)
MAX_RECSIZE = 255
MAX_LINES = 2**31 - 1
MAX_ISOTOPES = 32767

_POW10 = [float(f'1e{i}') for i in range(23)]
_last_flagged = 0
_last_chunks = (0, 0)


def last_flagged():
    """Records of the last make_tli(device=True) that the device flagged and the host parsed."""
    return _last_flagged


def last_chunks():
    """Chunks that went through each of the two pinned buffers (and streams) in the last
    make_tli(device=True)."""
    return _last_chunks


# ---------------------------------------------------------------------------------------------
# The host statement
# ---------------------------------------------------------------------------------------------
def decimal_fast_path_host(text):
    """(value, flagged) of one numeric field: the rule of the kernel (pb_linelist.hip, Decimal).

    The field is blanks, a sign, decimal digits with at most one point, an `e`/`E` exponent with
    an optional sign, blanks.  With w the integer of its digits (leading zeros dropped) and q its
    decimal exponent, w <= 2^53 and |q| <= 22 give double(w) * 1e q or double(w) / 1e -q, one
    correctly rounded operation on two exact operands: the bits of float(text).  Everything else
    is flagged and its value is NaN."""
    if isinstance(text, str):
        text = text.encode('latin-1', 'replace')
    LEAD, SIGN, INT, FRAC, EXP, EXPSIGN, EXPDIG, TRAIL, BAD = range(9)
    w = nsig = ndig = nfrac = ex = 0
    state, neg, eneg = LEAD, False, False
    for c in text:
        d = c - 48
        if 0 <= d < 10:
            if state <= FRAC:
                if state < INT:
                    state = INT
                ndig += 1
                nfrac += state == FRAC
                nsig += (w != 0 or d != 0)
                if nsig <= 19:
                    w = w * 10 + d
            elif state <= EXPDIG:
                state = EXPDIG
                ex = min(ex * 10 + d, 100000)
            else:
                state = BAD
        elif c == 32:
            if state in (INT, FRAC, EXPDIG):
                state = TRAIL
            elif state not in (LEAD, TRAIL):
                state = BAD
        elif c == 46:
            state = FRAC if state <= INT else BAD
        elif c in (101, 69):
            state = EXP if state in (INT, FRAC) and ndig > 0 else BAD
        elif c in (43, 45):
            if state == LEAD:
                state, neg = SIGN, c == 45
            elif state == EXP:
                state, eneg = EXPSIGN, c == 45
            else:
                state = BAD
        else:
            state = BAD
    q = (-ex if eneg else ex) - nfrac
    if not (ndig > 0 and state in (INT, FRAC, EXPDIG, TRAIL) and nsig <= 19 and w <= 2**53
            and -22 <= q <= 22):
        return float('nan'), True
    v = float(w) / _POW10[-q] if q < 0 else float(w) * _POW10[q]
    return (-v if neg else v), False


def binsearch_host(wave, target, ilo, ihi, searchup=True):
    """The record index of `target` among records ilo..ihi whose value wave(irec) rises: the
    search of the reference's readers (linelist/driver.py:79-132).  A bisection that keeps the
    upper half when wave(mid) <= target, then a walk over equal values: up while the next record
    is still below the target (searchup), or down while the previous one is still above it,
    stopping at either end of the range."""
    imin, imax = ilo, ihi
    while ihi - ilo > 1:
        mid = (ihi + ilo) // 2
        if wave(mid) > target:
            ihi = mid
        else:
            ilo = mid
    irec = ilo if searchup else ihi
    while irec != imin and irec != imax:
        if searchup:
            if not wave(irec + 1) < target:
                break
            irec += 1
        else:
            if not wave(irec - 1) > target:
                break
            irec -= 1
    return irec


def gf_host(wn, a21, g2):
    """gf = g2 * A21 * C1 / (8 pi c) / wn**2 as NumPy evaluates it (hitran.py:199, exomol.py:200):
    two products from the left, a division by the scalar, a division by wn * wn."""
    wn = np.asarray(wn, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.asarray(g2, np.float64) * np.asarray(a21, np.float64) * C1 / GF_DIVISOR / wn**2.0


class FieldError(ValueError):
    """A field that Python itself refuses: .record (within the bytes given) and .field."""

    def __init__(self, record, field, message):
        super().__init__(message)
        self.record, self.field, self.message = record, field, message


def _number(convert, text, record, field):
    try:
        return convert(text)
    except ValueError as e:
        raise FieldError(record, field, str(e)) from None


def _hitran_record(rec, i):
    """(wn, elow, a21, g2, iso) of one record with float() on the slices of hitran.py:178-182."""
    char = rec[2:3].decode('latin-1')
    if char not in HITRAN_ISO:
        raise FieldError(i, 'iso', f'unknown isotope character {char!r}')
    v = {name: _number(float, rec[a:b], i, name) for name, a, b in HITRAN_FIELDS}
    return v['wn'], v['elow'], v['a21'], v['g2'], HITRAN_ISO[char]


def parse_hitran_host(data, recsize):
    """wn, elow, a21, g2 [n] doubles and iso [n] int16 of the n = len(data) // recsize HITRAN
    records in `data` (bytes), record by record.  The elow filter is make_tli's."""
    n = len(data) // recsize
    wn, elow, a21, g2 = (np.zeros(n) for _ in range(4))
    iso = np.zeros(n, np.int16)
    data = bytes(data)
    for i in range(n):
        wn[i], elow[i], a21[i], g2[i], iso[i] = _hitran_record(
            data[i * recsize:(i + 1) * recsize], i)
    return wn, elow, a21, g2, iso


def _exomol_record(rec, i, energy, degeneracy):
    """(wn, elow, a21, g2) of one record: int(), int(), float() of its first three tokens
    (exomol.py:181) and the gather of exomol.py:198-201."""
    tokens = rec.split()
    if len(tokens) < 3:
        raise FieldError(i, 'token', f'{len(tokens)} tokens in the record, 3 are needed')
    up = _number(int, tokens[0], i, 'up')
    low = _number(int, tokens[1], i, 'low')
    a21 = _number(float, tokens[2], i, 'a21')
    for name, state in (('up', up), ('low', low)):
        if not 0 <= state < len(energy):
            raise FieldError(i, name, f'state id {state} outside the {len(energy)} states')
    return energy[up] - energy[low], energy[low], a21, float(degeneracy[up])


def parse_exomol_host(data, recsize, energy, degeneracy):
    """wn, elow, a21, g2 [n] doubles of the n = len(data) // recsize ExoMol transition records in
    `data` (bytes), record by record, with the states' energies and degeneracies dense in the
    state id."""
    n = len(data) // recsize
    wn, elow, a21, g2 = (np.zeros(n) for _ in range(4))
    data = bytes(data)
    for i in range(n):
        wn[i], elow[i], a21[i], g2[i] = _exomol_record(
            data[i * recsize:(i + 1) * recsize], i, energy, degeneracy)
    return wn, elow, a21, g2


# ---------------------------------------------------------------------------------------------
# The caller's data files
# ---------------------------------------------------------------------------------------------
def read_isotopes(path):
    """(molecule, hitran_iso, exomol_iso, ratio, mass) arrays of a file in the layout of the
    reference's isotopes.dat: five columns, `#` comments and blank lines skipped."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith('#'):
                rows.append(line.split()[:5])
    mol, hit, exo, ratio, mass = zip(*rows) if rows else ((),) * 5
    return (np.array(mol), np.array(hit), np.array(exo), np.array(ratio, np.float64),
            np.array(mass, np.float64))


def read_pf(path):
    """(pf [niso, ntemp], isotopes, temperatures) of a tabulated partition-function file: the
    isotope names on the line after `@ISOTOPES`, then after `@DATA` one line per temperature
    with the temperature and one value per isotope."""
    if not os.path.isfile(path):
        raise ValueError(f"Partition-function file '{path}' does not exist.")
    with open(path) as f:
        lines = [line.strip() for line in f]
    isotopes, rows, where = None, [], None
    for k, line in enumerate(lines):
        if where == 'isotopes':
            isotopes, where = line.split(), None
        elif where == 'data':
            if line:
                rows.append(line.split())
        elif line == '@ISOTOPES':
            where = 'isotopes'
        elif line == '@DATA':
            where = 'data'
    if isotopes is None or not rows:
        raise ValueError(f"Partition-function file '{path}' has no @ISOTOPES or no @DATA")
    table = np.array(rows, np.float64)
    if table.shape[1] != len(isotopes) + 1:
        raise ValueError(f"Partition-function file '{path}': {table.shape[1] - 1} columns for "
                         f'{len(isotopes)} isotopes')
    return table[:, 1:].T.copy(), list(isotopes), table[:, 0].copy()


def get_exomol_mol(path):
    """(molecule, isotope) of an ExoMol file name such as `14N-1H3__BYTe__...`: the elements in
    order with their counts ('NH3'), and the last digit of every atom's mass number, repeated
    by its count ('4111').  Restates tools/tools.py:846-900."""
    atoms = os.path.basename(path).split('_')[0].split('-')
    elements, isotope = [], ''
    for atom in atoms:
        m = re.match(r'([0-9]+)([a-z]+)([0-9]*)', atom, re.I)
        if m is None:
            raise ValueError(f"'{path}' does not follow the ExoMol naming convention")
        count = int(m.group(3)) if m.group(3) else 1
        elements += count * [m.group(2)]
        isotope += m.group(1)[-1:] * count
    molecule = ''
    for element, run in itertools.groupby(elements):
        n = len(list(run))
        molecule += element + (str(n) if n > 1 else '')
    return ('CO2' if molecule == 'OCO' else molecule), isotope


def exomol_states_file(trans):
    """The `.states` file of a `.trans` file (exomol.py:38-56): 'trans' becomes 'states' and the
    range suffix `__lo-hi` is dropped (in the file's name; the reference edits the whole path)."""
    folder, sfile = os.path.split(trans)
    sfile = sfile.replace('trans', 'states')
    if sfile.count('__') == 2:
        sfile = sfile.replace(sfile[sfile.rindex('__'):sfile.index('.')], '')
    return os.path.join(folder, sfile)


def read_states(sfile, device=False):
    """(energy, degeneracy) dense in the state id up to the largest one (ids may have gaps, which
    stay 0): the first three tokens of every line.  `<sfile>.bz2` is read when sfile is absent.
    device=True: the text is parsed and scattered on the device (partitions.read_states_device,
    pb_parse_states), with the same arrays bit for bit; a file whose lines differ in length is
    read here."""
    if device:
        from . import partitions
        path = sfile if os.path.isfile(sfile) else sfile + '.bz2'
        if not os.path.isfile(path):
            raise ValueError(f"Exomol file '{sfile}' does not exist")
        got = partitions.read_states_device(path)
        if got is not None:
            return got
    if os.path.isfile(sfile):
        with open(sfile, 'rb') as f:
            lines = f.readlines()
    elif os.path.isfile(sfile + '.bz2'):
        with bz2.open(sfile + '.bz2', 'rb') as f:
            lines = f.readlines()
    else:
        raise ValueError(f"Exomol file '{sfile}' does not exist")
    ids = np.zeros(len(lines), np.int64)
    e = np.zeros(len(lines))
    g = np.zeros(len(lines), np.int64)
    for i, line in enumerate(lines):
        tok = line.split()
        ids[i], e[i], g[i] = int(tok[0]), float(tok[1]), int(tok[2])
    nstates = int(ids.max()) + 1 if len(ids) else 0
    energy = np.zeros(nstates)
    degeneracy = np.zeros(nstates, np.int64)
    energy[ids] = e
    degeneracy[ids] = g
    return energy, degeneracy


# ---------------------------------------------------------------------------------------------
# Databases
# ---------------------------------------------------------------------------------------------
class _File:
    """One file of a database: its record size (the length of the first line with its
    terminator), its record count (file size // record size: a short tail is not a record) and
    the window search."""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise ValueError(f"Input database file '{path}' does not exist.")
        self.path = path
        with open(path, 'rb') as f:
            self.recsize = len(f.readline())
            f.seek(0, 2)
            self.nrec = f.tell() // self.recsize if self.recsize else 0

    def window(self, db, wn_low, wn_high):
        """(istart, istop) of the records to read, or None when the file does not overlap."""
        if self.nrec == 0:
            return None
        with open(self.path, 'rb') as f:
            def wave(irec):
                try:
                    return db._wave(self, f, irec)
                except FieldError as e:
                    raise ValueError(f'{self.path}: record {irec}: field {e.field}: '
                                     f'{e.message}') from None
            first, last = wave(0), wave(self.nrec - 1)
            if wn_low > last or wn_high < first:
                return None
            istart = binsearch_host(wave, wn_low, 0, self.nrec - 1, searchup=False)
            istop = binsearch_host(wave, wn_high, istart, self.nrec - 1, searchup=True)
        return istart, istop


class _Database:
    kind = None

    def __init__(self, files, molecule, isotopes, iso_mass, iso_ratio, partition):
        files = [files] if isinstance(files, (str, os.PathLike)) else list(files)
        if not files:
            raise ValueError('There are no input database files')
        self.files = [_File(os.fspath(f)) for f in files]
        self.molecule = molecule
        self.name = f'{self.kind} {molecule}'
        self.isotopes = [str(i) for i in isotopes]
        self.iso_mass = np.asarray(iso_mass, np.float64)
        self.iso_ratio = np.asarray(iso_ratio, np.float64)
        if not len(self.isotopes) == len(self.iso_mass) == len(self.iso_ratio):
            raise ValueError(f'{self.name}: isotopes, iso_mass and iso_ratio differ in length')
        if len(self.isotopes) > MAX_ISOTOPES:
            raise ValueError(f'{self.name}: {len(self.isotopes)} isotopes, a TLI file holds at '
                             f'most {MAX_ISOTOPES} per database')
        if isinstance(partition, str) and partition in ('tips', 'poly'):
            raise ValueError(
                f"partition='{partition}': the TIPS tables and the polynomial coefficients are "
                'data of the reference package and are not shipped; give a tabulated file '
                '(read_pf) or (temperatures, pf, isotopes)')
        self.partition = partition

    def getpf(self):
        """(temperatures, pf [niso, ntemp], isotope names)."""
        if isinstance(self.partition, (str, os.PathLike)):
            pf, iso, temps = read_pf(os.fspath(self.partition))
        else:
            temps, pf, iso = self.partition
        return (np.asarray(temps, np.float64), np.atleast_2d(np.asarray(pf, np.float64)),
                [str(i) for i in iso])


class Hitran(_Database):
    """HITRAN / HITEMP `.par` files of one molecule (one path or several: HITEMP splits a
    molecule by wavenumber).  `isotopes`, `iso_mass`, `iso_ratio` in the order of the record's
    isotope character: '1'..'9', '0', 'A', 'B'."""
    kind = 'HITRAN'

    def __init__(self, files, molecule, isotopes, iso_mass, iso_ratio, partition):
        super().__init__(files, molecule, isotopes, iso_mass, iso_ratio, partition)
        for f in self.files:
            if not HITRAN_END <= f.recsize <= MAX_RECSIZE:
                raise ValueError(f'{f.path}: records of {f.recsize} bytes are no HITRAN records '
                                 f'({HITRAN_END} ... {MAX_RECSIZE})')

    def _wave(self, file, f, irec):
        f.seek(irec * file.recsize + 3)
        return _number(float, f.read(12), irec, 'wn')


class Exomol(_Database):
    """ExoMol `.trans` files of one molecule, each with the `.states` file its name points to.
    The file's isotope is read from its name and looked up in `isotopes`; files of several
    isotopologues of one molecule are separate Exomol objects or one (make_tli merges objects of
    equal name either way).  device=True reads the `.states` files on the device (read_states);
    partition=(temps, pf, isotopes) may come straight from partitions.exomol_states."""
    kind = 'Exomol'

    def __init__(self, files, isotopes, iso_mass, iso_ratio, partition, device=False):
        files = [files] if isinstance(files, (str, os.PathLike)) else list(files)
        named = [get_exomol_mol(os.fspath(f)) for f in files]
        if len({m for m, _ in named}) > 1:
            raise ValueError(f'files of several molecules in one Exomol database: '
                             f'{sorted({m for m, _ in named})}')
        super().__init__(files, named[0][0] if named else None, isotopes, iso_mass, iso_ratio,
                         partition)
        states = {}
        for file, (_, iso) in zip(self.files, named):
            if not 5 <= file.recsize <= MAX_RECSIZE:
                raise ValueError(f'{file.path}: records of {file.recsize} bytes (5 ... '
                                 f'{MAX_RECSIZE})')
            if iso not in self.isotopes:
                raise ValueError(f"{file.path}: isotope '{iso}' is not among the isotopes "
                                 f'{self.isotopes} of {self.name}')
            file.iso = self.isotopes.index(iso)
            sfile = exomol_states_file(file.path)
            if sfile not in states:
                states[sfile] = read_states(sfile, device=device)
            file.energy, file.degeneracy = states[sfile]

    def _wave(self, file, f, irec):
        f.seek(irec * file.recsize)
        tok = f.readline().split()
        if len(tok) < 2:
            raise FieldError(irec, 'token', f'{len(tok)} tokens in the record')
        up, low = _number(int, tok[0], irec, 'up'), _number(int, tok[1], irec, 'low')
        for name, state in (('up', up), ('low', low)):
            if not 0 <= state < len(file.energy):
                raise FieldError(irec, name,
                                 f'state id {state} outside the {len(file.energy)} states')
        return file.energy[up] - file.energy[low]


# ---------------------------------------------------------------------------------------------
# Reading a window of a file
# ---------------------------------------------------------------------------------------------
def _located(path, istart, e):
    return ValueError(f'{path}: record {istart + e.record}: field {e.field}: {e.message}')


def _read_host(db, file, istart, istop):
    """wn, gf, elow, iso of the records istart..istop of one file, on the host."""
    with open(file.path, 'rb') as f:
        f.seek(istart * file.recsize)
        data = f.read((istop - istart + 1) * file.recsize)
    try:
        if db.kind == 'HITRAN':
            wn, elow, a21, g2, iso = parse_hitran_host(data, file.recsize)
        else:
            wn, elow, a21, g2 = parse_exomol_host(data, file.recsize, file.energy,
                                                  file.degeneracy)
            iso = np.full(len(wn), file.iso, np.int16)
    except FieldError as e:
        raise _located(file.path, istart, e) from None
    gf = gf_host(wn, a21, g2)
    if db.kind == 'HITRAN':
        good = elow > 0                 # lines with unknown Elow (hitran.py:202)
        wn, gf, elow, iso = wn[good], gf[good], elow[good], iso[good]
    return wn, gf, elow, iso


def _patch_flagged(db, file, istart, first, data, flags, columns):
    """The flagged records of one chunk, parsed on the host from the chunk's bytes and written
    into the device columns.  first: the chunk's first record within the window."""
    import torch
    rows = np.nonzero(flags)[0]
    values = np.zeros((len(rows), 5))
    for k, i in enumerate(rows):
        rec = bytes(data[i * file.recsize:(i + 1) * file.recsize])
        try:
            if db.kind == 'HITRAN':
                values[k] = _hitran_record(rec, first + i)
            else:
                values[k, :4] = _exomol_record(rec, first + i, file.energy, file.degeneracy)
                values[k, 4] = file.iso
        except FieldError as e:
            raise _located(file.path, istart, e) from None
    index = torch.from_numpy(rows + first).cuda()
    for j, name in enumerate(('wn', 'elow', 'a21', 'g2')):
        columns[name][index] = torch.from_numpy(values[:, j].copy()).cuda()
    columns['iso'][index] = torch.from_numpy(values[:, 4].astype(np.int16)).cuda()
    return len(rows)


class _Chunker:
    """Two pinned host buffers, two device text buffers and two streams: while one chunk is
    copied and parsed, the next is read from the file.  A chunk holds whole records."""

    def __init__(self, chunk_bytes):
        import torch
        from . import _device
        self.torch = torch
        self.nbytes = int(chunk_bytes)
        self.pinned = [torch.empty(self.nbytes, dtype=torch.uint8).pin_memory() for _ in (0, 1)]
        self.text = [torch.empty(self.nbytes, dtype=torch.uint8, device='cuda') for _ in (0, 1)]
        self.count = [torch.zeros(1, dtype=torch.int32, device='cuda') for _ in (0, 1)]
        self.count_h = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in (0, 1)]
        self.streams = _device.side_streams(2)
        self.used = [0, 0]                       # chunks that went through each buffer

    def run(self, source, nrec, recsize, launch, patch, short):
        """nrec records of recsize bytes read from `source` (readinto) through the two buffers;
        returns the number of flagged records.  launch(b, first, n, stream): enqueue the parse
        of the n records in self.text[b], records first .. first + n - 1 of the read, counting
        the flagged ones into self.count[b].  patch(b, first, n): called on the host, under the
        buffer's stream, when that count came back non-zero and while self.pinned[b] still holds
        the chunk's bytes; returns how many records it patched.  short(first, n): the exception
        for a source that ends inside the chunk."""
        torch = self.torch
        per_chunk = self.nbytes // recsize
        if per_chunk < 1:
            raise ValueError(f'chunk_bytes = {self.nbytes} holds no record of {recsize} bytes')
        flagged = 0
        pending = [None, None]                   # (event, first, n) of the chunk in each buffer
        main = torch.cuda.current_stream()

        def settle(b):
            nonlocal flagged
            if pending[b] is None:
                return
            event, first, n = pending[b]
            pending[b] = None
            event.synchronize()
            if int(self.count_h[b][0]):
                with torch.cuda.stream(self.streams[b]):
                    flagged += patch(b, first, n)
                self.streams[b].synchronize()

        ready = torch.cuda.Event()
        ready.record(main)                       # the columns exist before a side stream writes
        for k, first in enumerate(range(0, nrec, per_chunk)):
            b = k & 1
            settle(b)                            # the buffer's previous chunk is done with it
            n = min(per_chunk, nrec - first)
            view = memoryview(self.pinned[b].numpy())[:n * recsize]
            if source.readinto(view) != n * recsize:
                raise short(first, n)
            stream = self.streams[b]
            with torch.cuda.stream(stream):
                stream.wait_event(ready)
                self.text[b][:n * recsize].copy_(self.pinned[b][:n * recsize],
                                                 non_blocking=True)
                self.count[b].zero_()
                launch(b, first, n, torch.cuda.current_stream().cuda_stream)
                self.count_h[b].copy_(self.count[b], non_blocking=True)
                event = torch.cuda.Event()
                event.record(stream)
            pending[b] = (event, first, n)
            self.used[b] += 1
        settle(0)
        settle(1)
        for s in self.streams:
            main.wait_stream(s)
        return flagged

    def parse(self, db, file, istart, istop, columns):
        """Records istart..istop of `file` into `columns` (device tensors of the window's
        length); returns the number of flagged records."""
        torch = self.torch
        from ._device import _ptr
        from ._capi import call
        recsize = file.recsize
        if db.kind == 'Exomol':
            energy = torch.from_numpy(file.energy).cuda()
            degeneracy = torch.from_numpy(file.degeneracy.astype(np.float64)).cuda()

        def launch(b, first, n, stream):
            out = [_ptr(columns[c][first:first + n])
                   for c in ('wn', 'elow', 'a21', 'g2', 'iso', 'flags')]
            if db.kind == 'HITRAN':
                call('pb_parse_hitran', _ptr(self.text[b]), n, recsize, *out,
                     _ptr(self.count[b]), stream)
            else:
                call('pb_parse_exomol', _ptr(self.text[b]), n, recsize, _ptr(energy),
                     _ptr(degeneracy), len(file.energy), file.iso, *out,
                     _ptr(self.count[b]), stream)

        def patch(b, first, n):
            flags = columns['flags'][first:first + n].cpu().numpy()
            return _patch_flagged(db, file, istart, first,
                                  self.pinned[b].numpy()[:n * recsize], flags, columns)

        def short(first, n):
            return ValueError(f'{file.path}: the file ended inside record '
                              f'{istart + first} ... {istart + first + n - 1}')

        with open(file.path, 'rb') as f:
            f.seek(istart * recsize)
            return self.run(f, istop - istart + 1, recsize, launch, patch, short)


def _read_device(db, file, istart, istop, chunker):
    """wn, gf, elow, iso of the records istart..istop of one file, as device tensors."""
    import torch
    from ._device import _ptr, _stream
    from ._capi import call
    global _last_flagged
    n = istop - istart + 1
    columns = {c: torch.empty(n, dtype=torch.float64, device='cuda')
               for c in ('wn', 'elow', 'a21', 'g2')}
    columns['iso'] = torch.empty(n, dtype=torch.int16, device='cuda')
    columns['flags'] = torch.empty(n, dtype=torch.uint8, device='cuda')
    _last_flagged += chunker.parse(db, file, istart, istop, columns)
    gf = torch.empty(n, dtype=torch.float64, device='cuda')
    # after the patch, by the same kernel statement for every record
    call('pb_linelist_gf', _ptr(columns['wn']), _ptr(columns['a21']), _ptr(columns['g2']), n,
         C1, GF_DIVISOR, _ptr(gf), _stream())
    wn, elow, iso = columns['wn'], columns['elow'], columns['iso']
    if db.kind == 'HITRAN':
        good = elow > 0
        wn, gf, elow, iso = wn[good], gf[good], elow[good], iso[good]
    return wn, gf, elow, iso


# ---------------------------------------------------------------------------------------------
# make_tli
# ---------------------------------------------------------------------------------------------
# device bytes per line of a database while it is sorted: the parsed columns (4 doubles, int16,
# flags) and gf, the concatenated copies (3 doubles, int16), and two rounds of torch.sort on a
# key with its int64 permutation plus the gathered columns
_DEVICE_BYTES_PER_LINE = (4 * 8 + 2 + 1 + 8) + (3 * 8 + 2) + 2 * (8 + 8 + 8) + (3 * 8 + 2)


def make_tli(databases, tlifile, wn_low=None, wn_high=None, wl_low=None, wl_high=None,
             device=True, chunk_bytes=256 << 20):
    """Write the TLI file of the line lists in `databases` (Hitran / Exomol objects; objects of
    equal name become one TLI database) between wn_low and wn_high in cm-1, or wl_low and wl_high
    in cm.  Returns the list of database dicts that tli.write_tli takes, as host arrays.

    device=False: the host route.  chunk_bytes: the size of each of the two pinned buffers the
    file's text passes through; a chunk holds whole records."""
    global _last_flagged, _last_chunks
    if isinstance(databases, _Database):
        databases = [databases]
    if not databases:
        raise ValueError('There are no input databases')
    if wn_low is None:
        if wl_high is None:
            raise ValueError('Undefined low wavenumber boundary (wn_low, or wl_high)')
        wn_low = 1.0 / wl_high
    if wn_high is None:
        if wl_low is None:
            raise ValueError('Undefined high wavenumber boundary (wn_high, or wl_low)')
        wn_high = 1.0 / wl_low
    wn_low, wn_high = float(wn_low), float(wn_high)

    names = []
    for db in databases:
        if db.name not in names:
            names.append(db.name)
    if len(names) > MAX_ISOTOPES:
        raise ValueError(f'{len(names)} databases, a TLI file holds at most {MAX_ISOTOPES}')

    # the windows of every file, before anything is read or launched
    plan, total, largest = [], 0, 0
    for name in names:
        members = [db for db in databases if db.name == name]
        last = members[-1]                       # the reference's `this_db`: names, pf of the last
        reads = []
        for db in members:
            for file in db.files:
                win = file.window(db, wn_low, wn_high)
                if win is not None:
                    reads.append((db, file) + win)
        nlines = sum(istop - istart + 1 for _, _, istart, istop in reads)
        if not reads:
            raise ValueError(
                f"{name}: none of its files overlaps the requested wavenumber range "
                f'({wn_low:.2f}--{wn_high:.2f} cm-1)')
        pf_iso = last.getpf()[2]
        missing = sorted({db.isotopes[file.iso] for db, file, _, _ in reads
                          if db.kind == 'Exomol'} - set(pf_iso))
        if missing:
            raise ValueError('No partition functions found for these isotopes of the '
                             f'{last.molecule} line list: {missing}')
        plan.append((last, reads))
        total += nlines
        largest = max(largest, nlines)
    if total > MAX_LINES:
        raise ValueError(f'{total} lines in the window, a TLI file holds at most {MAX_LINES}')

    chunker = None
    if device:
        import torch
        from . import _device
        _device.require_gpu()
        # no buffer larger than the largest window of a file
        buffer_bytes = min(int(chunk_bytes), max(
            (b - a + 1) * file.recsize for _, reads in plan for _, file, a, b in reads))
        need = largest * _DEVICE_BYTES_PER_LINE + 2 * buffer_bytes
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            raise ValueError(f'the columns and the sort scratch of {largest} lines and two '
                             f'chunks of {buffer_bytes} bytes need {need} bytes of device '
                             f'memory, {free} are free')
        _last_flagged = 0
        chunker = _Chunker(buffer_bytes)

    out, iso_offset = [], 0
    for last, reads in plan:
        parts = [(_read_device(db, file, a, b, chunker) if device else
                  _read_host(db, file, a, b)) for db, file, a, b in reads]
        if device:
            wn, gf, elow, iso = (torch.cat([p[j] for p in parts]) for j in range(4))
            # stable, by isotope, then wavenumber, then input order
            order = torch.sort(wn, stable=True)[1]
            order = order[torch.sort(iso[order], stable=True)[1]]
            wn, gf, elow, iso = (t[order].cpu().numpy() for t in (wn, gf, elow, iso))
        else:
            wn, gf, elow, iso = (np.concatenate([p[j] for p in parts]) for j in range(4))
            order = np.lexsort((wn, iso))        # stable: isotope, wavenumber, input order
            wn, gf, elow, iso = wn[order], gf[order], elow[order], iso[order]
        if len(wn) == 0:
            raise ValueError(f'{last.name}: no line with a known Elow in the requested '
                             f'wavenumber range ({wn_low:.2f}--{wn_high:.2f} cm-1)')
        # isotopes without lines are filtered out; the file's index counts the remaining ones
        unique_iso, iso_idx = np.unique(iso, return_inverse=True)
        if unique_iso[-1] >= len(last.isotopes):
            raise ValueError(f'{last.name}: lines of isotope index {int(unique_iso[-1])}, but '
                             f'only {len(last.isotopes)} isotopes were given')
        iso_names = [last.isotopes[i] for i in unique_iso]
        temps, partition, pf_iso = last.getpf()
        missing = [i for i in iso_names if i not in pf_iso]
        if missing:
            raise ValueError('No partition functions found for these isotopes of the '
                             f'{last.molecule} line list: {missing}')
        out.append(dict(
            name=last.name, molecule=last.molecule, temperatures=temps, isotopes=iso_names,
            iso_mass=last.iso_mass[unique_iso], iso_ratio=last.iso_ratio[unique_iso],
            partition=partition[[pf_iso.index(i) for i in iso_names]],
            wn=wn, iso_id=(iso_idx + iso_offset).astype(np.int32), elow=elow, gf=gf))
        iso_offset += len(iso_names)
    if device:
        _last_chunks = tuple(chunker.used)
    _tli.write_tli(tlifile, out, wn_min=wn_low, wn_max=wn_high)
    return out
