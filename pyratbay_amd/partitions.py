"""Partition functions: the reference's `pf` step (pyratbay/opacity/partitions/partitions.py:
check_exomol_files, exomol_pf, exomol_states, kurucz; io.write_pf), with its argument names, its
return order (pf [niso, ntemp], isotopes, temps) and its error texts.

    from pyratbay_amd import partitions as pf, linelist as ll
    q, isotopes, temps = pf.exomol_states(['14N-1H3__BYTe.states.bz2'], 5.0, 5000.0, 5.0)
    nh3 = ll.Exomol(trans_files, isotopes=[...], iso_mass=[...], iso_ratio=[...],
                    partition=(temps, q, isotopes))

exomol_states evaluates Q_i(T) = sum_j g_j exp(-C2 E_j / T) over every state of a `.states` file
for every temperature of the grid.  The reference reads the file with one split() per line in a
Python loop and runs one NumPy pass per temperature.  Here the file's bytes go to the device in
chunks through the two pinned buffers and streams of linelist.make_tli, one lane parses one record
(csrc/pb_partitions.hip: pb_parse_states), the energies and degeneracies stay on the device and
pb_pf_states sums them for all temperatures at once.  `device=False` is the host statement: the
reference's loop and `np.sum(degeneracy*np.exp(-C2*energy/temps[j]))`.  It needs no GPU.

The device takes a record only when its three tokens are on the exact fast path of the conversion
and the reference's two readings of a line agree on it (`line[12:32].split()` of partitions.py:407
and `line.split()[0:3]` of exomol.py): parse_states_host is the kernel's rule in Python.  Every
other record is flagged and the host reads it from the bytes it still holds; last_flagged() says
how many of the last call were.  A file whose lines do not all have one length takes the host
route as a whole.

exomol_pf, kurucz and write_pf run on the host: their files are small.  The TIPS table is data of
the reference package and is not shipped: tips() refuses.
"""
import bz2
import io
import os
import warnings

import numpy as np

from . import linelist as _ll

# the reference's constants (constants/astrophysical_constants.py:67-69): scipy.constants' h * 1e7,
# k * 1e7 (exact since 2019) and c * 1e2
_H = 6.62607015e-34 * 1e7
_K = 1.380649e-23 * 1e7
C2 = _H * _ll._C / _K

# flag bits of a record (include/pbhip.h, PB_LL_STATES_*)
STATES_FLAGS = dict(id=1, energy=2, g=4, token=8, layout=16)
STATES_SCAN = 33                 # the kernel reads bytes 0 ... 32 of a record
MIN_RECSIZE, MAX_RECSIZE = STATES_SCAN, _ll.MAX_RECSIZE
ID_DIGITS, G_DIGITS = 18, 15
MAX_TEMPS = 65536
MAX_STATES = 2**31 - 1

_last_flagged = 0
_last_routes = []


def last_flagged():
    """Records that the device flagged and the host read in the last exomol_states(device=True)
    (all its files together) or the last linelist.read_states(device=True)."""
    return _last_flagged


def routes():
    """'device' or 'host' for each file of the last exomol_states call: a file whose lines do not
    all have one length (or are shorter than 33 or longer than 255 bytes) is read by the host's
    Python loop, which takes minutes where the device takes a tenth of a second."""
    return list(_last_routes)


# ---------------------------------------------------------------------------------------------
# The host statement
# ---------------------------------------------------------------------------------------------
def _unsigned_host(token, maxdig):
    body = token[1:] if token[:1] == b'+' else token
    if 1 <= len(body) <= maxdig and body.isdigit():
        return int(body), False
    return -1, True


def states_record_host(rec, recsize):
    """(id, energy, degeneracy, flags) of one record of recsize bytes: the rule of k_parse_states.

    Bytes 0 ... 32 are cut at blanks (byte recsize - 1, the line feed, counts as one).  The first
    three tokens are an integer (an optional '+', 1 ... 18 digits), a decimal on the fast path
    (linelist.decimal_fast_path_host) and an integer (1 ... 15 digits).  `token`: fewer than three
    tokens end within those bytes, or a white-space byte other than the blank lies there.
    `layout`: byte recsize - 1 is no line feed or a line feed lies earlier; the id ends behind
    byte 11, the energy starts before byte 12, the degeneracy runs past byte 31 or a fourth token
    starts before byte 32.  A flagged token is -1 / NaN, all three with `token` or `layout`."""
    F = STATES_FLAGS
    fl = 0
    if rec[recsize - 1:recsize] != b'\n' or b'\n' in rec[:recsize - 1]:
        fl |= F['layout']
    k, in_token, tokens = 0, False, [b'', b'', b'']
    for i in range(STATES_SCAN):
        c = rec[i]
        blank = c == 32 or i == recsize - 1
        if blank or 9 <= c <= 13:
            if not blank:
                fl |= F['token']
            if in_token:
                if k == 0 and i > 12:
                    fl |= F['layout']
                k += 1
                in_token = False
        else:
            if not in_token:
                in_token = True
                if (k == 1 and i < 12) or (k == 3 and i < 32):
                    fl |= F['layout']
            if k < 3:
                tokens[k] += rec[i:i + 1]
    if k < 3:
        fl |= F['layout'] if in_token else F['token']
    if fl & (F['token'] | F['layout']):
        return -1, float('nan'), float('nan'), fl
    ident, bad_id = _unsigned_host(tokens[0], ID_DIGITS)
    energy, bad_e = _ll.decimal_fast_path_host(tokens[1])
    g, bad_g = _unsigned_host(tokens[2], G_DIGITS)
    fl |= F['id'] * bad_id | F['energy'] * bad_e | F['g'] * bad_g
    return ident, energy, (float('nan') if bad_g else float(g)), fl


def parse_states_host(data, recsize):
    """id [n] int64, energy, degeneracy [n] doubles and flags [n] uint8 of the n = len(data) //
    recsize records in `data` (bytes), record by record, as pb_parse_states writes them."""
    n = len(data) // recsize
    ids = np.zeros(n, np.int64)
    energy, degeneracy = np.zeros(n), np.zeros(n)
    flags = np.zeros(n, np.uint8)
    data = bytes(data)
    for i in range(n):
        ids[i], energy[i], degeneracy[i], flags[i] = states_record_host(
            data[i * recsize:(i + 1) * recsize], recsize)
    return ids, energy, degeneracy, flags


def temperature_grid(tmin, tmax, tstep):
    """The reference's two statements (partitions.py:390-391)."""
    ntemps = int((tmax-tmin)/tstep) + 1
    temps = np.linspace(tmin, tmin + (ntemps-1)*tstep, ntemps)
    return temps


def states_partition_host(energy, degeneracy, temps):
    """Q [ntemp] as the reference states it (partitions.py:409-410)."""
    temps = np.asarray(temps, np.float64)
    pf = np.zeros(len(temps))
    for j in range(len(temps)):
        pf[j] = np.sum(degeneracy*np.exp(-C2*energy/temps[j]))
    return pf


def _open_states(path, mode):
    return bz2.open(path, mode) if path.endswith('.bz2') else open(path, mode)


def read_states_pf_host(path):
    """(energy, degeneracy) of every line of a `.states` file, in file order, as the reference's
    `pf` step reads a line: the two tokens of its bytes 12 ... 31, a float and an int.  A line
    with another number of tokens there, or with tokens of another kind, is a ValueError."""
    energy, degeneracy = [], []
    with _open_states(path, 'rt') as f:
        for line in f:
            e, g = line[12:32].split()
            energy.append(float(e))
            degeneracy.append(int(g))
    return np.array(energy, np.float64), np.array(degeneracy, int)


# ---------------------------------------------------------------------------------------------
# The device route
# ---------------------------------------------------------------------------------------------
class _HostRoute(Exception):
    """The file is the host's: ragged lines, or a value the device columns cannot hold."""


def _reread(rec, reading):
    """(id, energy, degeneracy) of a flagged record by the reference's reading of that route:
    'pf' takes the two tokens of bytes 12 ... 31, 'states' the record's first three tokens.  A
    record whose line feed is not its last byte and only that one makes the file the host's."""
    if rec[-1:] != b'\n' or b'\n' in rec[:-1]:
        raise _HostRoute
    if reading == 'pf':
        e, g = rec[12:32].split()
        ident, e, g = -1, float(e), int(g)
    else:
        tok = rec.split()
        ident, e, g = int(tok[0]), float(tok[1]), int(tok[2])
    if abs(g) >= 2**53 or abs(ident) >= 2**63:
        raise _HostRoute
    return ident, e, g


def parse_states_device(path, reading='pf', chunk_bytes=256 << 20):
    """(id, energy, degeneracy) device tensors [nlines] of a `.states` or `.states.bz2` file in
    file order, flagged records read by the host (`reading`: see _reread) and added to
    last_flagged(), or None when the file takes the host route: lines of more than one length,
    or of fewer than 33 or more than 255 bytes.  The chunks go through linelist._Chunker.run."""
    import torch
    from . import _device
    from ._capi import call
    from ._device import _ptr
    global _last_flagged
    _device.require_gpu()
    if path.endswith('.bz2'):
        with bz2.open(path, 'rb') as f:
            source = io.BytesIO(f.read())
        size = source.getbuffer().nbytes
    else:
        source = open(path, 'rb')
        size = os.path.getsize(path)
    with source:
        recsize = len(source.readline())
        source.seek(0)
        if size == 0:
            return (torch.zeros(0, dtype=torch.int64, device='cuda'),
                    torch.zeros(0, dtype=torch.float64, device='cuda'),
                    torch.zeros(0, dtype=torch.float64, device='cuda'))
        if not MIN_RECSIZE <= recsize <= MAX_RECSIZE or size % recsize:
            return None
        n = size // recsize
        if n > MAX_STATES:
            return None
        chunker = _ll._Chunker(max(recsize, min(int(chunk_bytes), size)))
        cols = dict(id=torch.empty(n, dtype=torch.int64, device='cuda'),
                    energy=torch.empty(n, dtype=torch.float64, device='cuda'),
                    g=torch.empty(n, dtype=torch.float64, device='cuda'),
                    flags=torch.empty(n, dtype=torch.uint8, device='cuda'))

        def launch(b, first, m, stream):
            out = [_ptr(cols[c][first:first + m]) for c in ('id', 'energy', 'g', 'flags')]
            call('pb_parse_states', _ptr(chunker.text[b]), m, recsize, *out,
                 _ptr(chunker.count[b]), stream)

        def patch(b, first, m):
            rows = np.nonzero(cols['flags'][first:first + m].cpu().numpy())[0]
            data = chunker.pinned[b].numpy()
            values = [_reread(bytes(data[i * recsize:(i + 1) * recsize]), reading) for i in rows]
            index = torch.from_numpy(rows + first).cuda()
            for c, (k, dtype) in (('id', (0, torch.int64)), ('energy', (1, torch.float64)),
                                  ('g', (2, torch.float64))):
                cols[c][index] = torch.tensor([v[k] for v in values], dtype=dtype).cuda()
            return len(rows)

        try:
            flagged = chunker.run(source, n, recsize, launch, patch, lambda first, m: _HostRoute())
        except _HostRoute:
            torch.cuda.synchronize()
            return None
    _last_flagged += flagged
    return cols['id'], cols['energy'], cols['g']


def states_partition(energy, degeneracy, temps):
    """Q [ntemp] = sum_j degeneracy[j] * exp(-C2 * energy[j] / temps[t]): device tensors of doubles
    in, a device tensor out (pb_pf_states).  The same bits on every call and stream."""
    import ctypes
    import torch
    from ._capi import call
    from ._device import _ptr, _stream
    for name, t in (('energy', energy), ('degeneracy', degeneracy), ('temps', temps)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64
                and t.dim() == 1):
            raise ValueError(f'states_partition: {name} must be a 1D device tensor of doubles')
    if energy.shape != degeneracy.shape:
        raise ValueError(f'states_partition: {energy.numel()} energies and '
                         f'{degeneracy.numel()} degeneracies')
    nstates, ntemp = energy.numel(), temps.numel()
    if nstates > MAX_STATES or ntemp > MAX_TEMPS:
        raise ValueError(f'states_partition: {nstates} states x {ntemp} temperatures: at most '
                         f'{MAX_STATES} x {MAX_TEMPS}')
    energy, degeneracy, temps = energy.contiguous(), degeneracy.contiguous(), temps.contiguous()
    sizes = (ctypes.c_int64 * 2)()
    call('pb_pf_states_work', nstates, ntemp, sizes)
    q = torch.empty(ntemp, dtype=torch.float64, device=temps.device)
    work = torch.empty(max(int(sizes[0]), 1), dtype=torch.float64, device=temps.device)
    if ntemp:
        call('pb_pf_states', _ptr(energy) if nstates else None,
             _ptr(degeneracy) if nstates else None, nstates, _ptr(temps), ntemp, C2, _ptr(q),
             _ptr(work), _stream())
    return q


def read_states_device(path, chunk_bytes=256 << 20):
    """linelist.read_states on the device: (energy, degeneracy) host arrays dense in the state id,
    or None when the file takes the host route (parse_states_device, or ids that NumPy's
    assignment treats specially: negative ones and repeated ones)."""
    import torch
    global _last_flagged
    _last_flagged = 0
    got = parse_states_device(path, 'states', chunk_bytes)
    if got is None:
        return None
    ids, e, g = got
    if ids.numel() == 0:
        return np.zeros(0), np.zeros(0, np.int64)
    if int(ids.min()) < 0 or int(ids.max()) >= MAX_STATES:
        return None
    if not bool((ids[1:] > ids[:-1]).all()) and torch.unique(ids).numel() != ids.numel():
        return None
    nstates = int(ids.max()) + 1
    energy = torch.zeros(nstates, dtype=torch.float64, device='cuda')
    degeneracy = torch.zeros(nstates, dtype=torch.int64, device='cuda')
    energy[ids] = e
    degeneracy[ids] = g.to(torch.int64)
    return energy.cpu().numpy(), degeneracy.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# The front end: the reference's interface, error texts and output bytes
# ---------------------------------------------------------------------------------------------
def write_pf(pffile, pf, isotopes, temp, header=None):
    """Write the table pf [niso, ntemp] to a partition-function file of the layout
    linelist.read_pf reads: the optional header, the isotope names in columns of 13 after
    `@ISOTOPES`, and after `@DATA` one line per temperature, `%7.1f` and `%.7e` values."""
    table = np.asarray(pf)
    if table.shape[:1] != (len(isotopes),):
        raise ValueError('Shape of the partition-function array does not '
                         'match with the number of isotopes.')
    if table.shape[1:2] != (len(temp),):
        raise ValueError('Shape of the partition-function array does not '
                         'match with the number of temperature samples.')
    names = '  '.join(f'{str(iso):13s}' for iso in isotopes)
    text = [header or '',
            f'@ISOTOPES\n            {names}\n\n',
            '# Temperature (K), partition function for each isotope:\n@DATA\n']
    for k, t in enumerate(temp):
        row = '  '.join(f'{q:.7e}' for q in table[:, k])
        text.append(f'  {t:7.1f}   {row}\n')
    with open(pffile, 'w') as f:
        f.writelines(text)


def _file_kind(name):
    name = name.strip()
    if name.endswith('.pf'):
        return 'pf'
    return 'states' if name.endswith(('.states', '.states.bz2')) else ''


def check_exomol_files(files):
    """(file_type, molecule, isotopes) of a list of ExoMol file names: file_type is 'pf' when
    every name ends in `.pf`, 'states' when every name ends in `.states` or `.states.bz2`, and ''
    for a mixture; molecule and isotopes come from the names (linelist.get_exomol_mol), and
    names of two molecules are refused."""
    kinds = {_file_kind(file) for file in files}
    file_type = kinds.pop() if len(kinds) == 1 else '' if kinds else 'pf'
    molecule, isotopes = '', []
    for file in files:
        name, iso = _ll.get_exomol_mol(file)
        if isotopes and name != molecule:
            raise ValueError('All files must correspond to the same molecule')
        molecule = name
        isotopes.append(iso)
    return file_type, molecule, isotopes


def _finish(kind, source, molecule, pf, isotopes, temps, outfile):
    """The common end of the three readers: write the table when asked (`'default'`:
    PF_<kind>_<molecule>.dat) under the reference's header, and say so."""
    if outfile is None:
        return
    if outfile == 'default':
        outfile = f'PF_{kind}_{molecule}.dat'
    write_pf(outfile, pf, isotopes, temps,
             f'# This file incorporates the tabulated {molecule} partition-function data\n'
             f'# from {source}\n\n')
    print(f"\nWritten partition-function file:\n  '{outfile}'\n"
          f'for molecule {molecule}, with isotopes {isotopes},\n'
          f'and temperature range {temps[0]:.0f}--{temps[-1]:.0f} K.')


def exomol_pf(files, outfile=None):
    """(pf [niso, ntemp], isotopes, temps) of ExoMol `.pf` files of one molecule (one path or a
    list): two columns, temperature and Q.  Files of different lengths are cut to the shortest,
    with a warning, if they agree on the temperatures up to there, and refused if not.
    outfile: write the table (`'default'`: PF_exomol_<molecule>.dat)."""
    files = [files] if isinstance(files, str) else files
    file_type, molecule, isotopes = check_exomol_files(files)
    if file_type != 'pf':
        raise ValueError("All input files must be exomol '.pf' files")
    tables = [np.loadtxt(file, ndmin=2) for file in files]
    ntemp = min(len(table) for table in tables)
    temps = tables[0][:ntemp, 0].copy()
    if any(len(table) != ntemp for table in tables):
        if not all(np.array_equal(table[:ntemp, 0], temps) for table in tables):
            raise ValueError('Temperature sampling in PF files are not compatible')
        warnings.warn('Length of PF files do not match. Trimming to shorter size')
    pf = np.array([table[:ntemp, 1] for table in tables], np.float64).reshape(len(files), ntemp)
    _finish('exomol', 'Exomol', molecule, pf, isotopes, temps, outfile)
    return pf, isotopes, temps


def exomol_states(files, tmin, tmax, tstep, outfile=None, device=True,
                  chunk_bytes=256 << 20):
    """(pf [niso, ntemp], isotopes, temps) from ExoMol `.states` / `.states.bz2` files of one
    molecule (one path or a list), sampled from tmin to tmax in steps of tstep.  outfile: write
    the table (`'default'`: PF_exomol_<molecule>.dat).  device=False: the host statement.
    last_flagged() counts the records of this call that the host read; routes() says which file
    went which way."""
    global _last_flagged, _last_routes
    files = [files] if isinstance(files, str) else files
    file_type, molecule, isotopes = check_exomol_files(files)
    if file_type != 'states':
        raise ValueError("All input files must be exomol '.states' files")
    temps = temperature_grid(tmin, tmax, tstep)
    if device:
        import torch
        from . import _device
        _device.require_gpu()
        if len(temps) > MAX_TEMPS:
            raise ValueError(f'{len(temps)} temperatures, the device takes at most {MAX_TEMPS}')
        _last_flagged = 0
        temps_d = torch.from_numpy(temps).cuda()
    pf = np.zeros((len(files), len(temps)))
    routes = []
    for row, path in zip(pf, files):
        columns = parse_states_device(path, 'pf', chunk_bytes) if device else None
        routes.append('host' if columns is None else 'device')
        if columns is None:
            row[:] = states_partition_host(*read_states_pf_host(path), temps)
        else:
            row[:] = states_partition(columns[1], columns[2], temps_d).cpu().numpy()
    _last_routes = routes
    _finish('exomol', 'Exomol', molecule, pf, isotopes, temps, outfile)
    return pf, isotopes, temps


# the two layouts kurucz() serves: the word in the file's name, the molecule, the lines in front
# of the table, the isotope of each column
_KURUCZ = (
    ('h2o', 'H2O', 'h2o/h2opartfn.dat', 6, ('1H1H16O', '1H1H17O', '1H1H18O', '1H2H16O')),
    ('tio', 'TiO', 'tio/tiopart.dat', 1, ('66', '76', '86', '96', '06')),
)


def kurucz(pf_file, outfile=None, type_flag='as_exomol'):
    """(pf [niso, ntemp], isotopes, temp) of a partition-function file from Kurucz's site: the
    H2O layout (`h2o` in the file's name: h2opartfn.dat) or the TiO layout (`tio`: tiopart.dat),
    a temperature column and one column per isotope.  outfile: write the table (`'default'`:
    PF_kurucz_<molecule>.dat)."""
    layout = [entry for entry in _KURUCZ if entry[0] in pf_file]
    if not layout:
        raise ValueError('Invalid Kurucz partition-function file.')
    _, molecule, page, nskip, isotopes = layout[0]
    table = np.loadtxt(pf_file, skiprows=nskip, ndmin=2)
    temp, pf = table[:, 0].copy(), table[:, 1:].T.copy()
    isotopes = list(isotopes)
    _finish('kurucz', f'http://kurucz.harvard.edu/molecules/{page}', molecule, pf, isotopes,
            temp, outfile)
    return pf, isotopes, temp


def tips(molecule, isotopes=None, outfile=None, db_type='as_exomol'):
    """Refused: the TIPS 2021 table is data of the reference package and is not shipped."""
    raise ValueError(
        f"tips('{molecule}'): the TIPS 2021 table is data of the reference package and is not "
        'shipped; give a tabulated file (linelist.read_pf) or compute the partition function '
        'from ExoMol states (exomol_states), ExoMol .pf files (exomol_pf) or Kurucz files '
        '(kurucz)')


