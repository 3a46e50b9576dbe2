"""Cases of the partition-function tests (test_partitions_cpu.py, test_gpu_partitions.py): the
fixture inputs of g33_partitions.npz as files, builders of `.states` records, the constructed
records that must be flagged, and the exact value and the error bound of Q(T)."""
import atexit
import decimal
import os
import shutil
import tempfile

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_g33 = None


def g33():
    global _g33
    if _g33 is None:
        with np.load(os.path.join(GOLDEN, 'g33_partitions.npz')) as f:
            _g33 = {k: f[k] for k in f.files}
    return _g33


def _write_inputs():
    """The reference's mock inputs, held in g33 as bytes, as files under their own names in a
    scratch directory that lives as long as the process."""
    folder = tempfile.mkdtemp(prefix='pb_partitions_')
    atexit.register(shutil.rmtree, folder, ignore_errors=True)
    for key, raw in g33().items():
        if key.startswith('input_'):
            raw.tofile(os.path.join(folder, key[len('input_'):]))
    return folder


INPUT_DIR = _write_inputs()


def path(name):
    return os.path.join(INPUT_DIR, name)


NH3 = [path('14N-1H3__MockBYTe.states'), path('15N-1H3__MockBYTe-15.states')]
HCN = [path('1H-12C-14N__MockHarris.states')]
STATES = dict(nh3=NH3, hcn=HCN)
RECSIZE = {NH3[0]: 139, NH3[1]: 135, HCN[0]: 86}
GRIDS = dict(a=(100.0, 1500.0, 100.0), b=(5.0, 5000.0, 5.0))
KURUCZ = dict(h2o=path('mock_h2opartfn.dat'), tio=path('mock_tiopart.dat'))
PF_A, PF_B, PF_SHORT, PF_SHIFTED = (path(n) for n in (
    '1H-12C-14N__GenA.pf', '1H-13C-14N__GenB.pf', '1H-12C-15N__GenShort.pf',
    '1H-13C-15N__GenShifted.pf'))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_columns(got, want):
    """Equal bit for bit, NaN where the other side has NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(bits(got[~nan]), bits(want[~nan]))


# ---------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------
def states_record(ident, energy, g, recsize=139, head=None):
    """One `.states` record of recsize bytes: id right-justified in bytes 0-11, the energy in
    13-24, the degeneracy in 26-31 (ExoMol's `%12d %12.6f %6d`), then quantum numbers, a line
    feed.  head: the text of bytes 0 ... 31 (or longer) instead."""
    if head is None:
        head = f'{ident:>12} {energy:>12} {g:>6}'
        assert len(head) == 32, head
    tail = '  1  +  e  0  0  0'
    body = (head + tail)[:recsize - 1].ljust(recsize - 1)
    return body.encode('latin-1') + b'\n'


def random_states(rng, n, recsize, first_id=1):
    """n clean records with random energies `%12.6f` and degeneracies, ids rising."""
    energy = np.round(rng.uniform(0.0, 30000.0, n), 6)
    g = rng.integers(1, 1000, n)
    return b''.join(states_record(first_id + i, f'{energy[i]:.6f}', int(g[i]), recsize)
                    for i in range(n))


F = dict(id=1, energy=2, g=4, token=8, layout=16)

# (what it is, bytes 0 ... 31 or more of the record, the flag bits it must get in a record of
# more than 36 bytes: a shorter record cuts the longer heads)
FLAGGED = [
    ('a 17-digit energy, beyond 2^53', '          1 12345678901234567 18', F['energy']),
    ('a 20-digit energy: no third token ends by byte 32',
     '          1 12345678901234567890 18', F['token']),
    ('an exponent beyond +22', f'{1:>12} {"1.5e+24":>12} {18:>6}', F['energy']),
    ('an exponent beyond -22', f'{1:>12} {"1.5e-25":>12} {18:>6}', F['energy']),
    ('NaN as the energy', f'{2:>12} {"NaN":>12} {18:>6}', F['energy']),
    ('inf as the energy', f'{3:>12} {"inf":>12} {18:>6}', F['energy']),
    ('a tab inside a token: four tokens', f'{4:>12} {"6330.8":>6}\t{"75419":<5} {18:>6}',
     F['token'] | F['layout']),
    ('a two-token line', f'{5:>12} {"6330.875419":>12} {"":>6}   ', F['token']),
    ('an energy token that runs past byte 31', f'{6:>12} {"":>9}{"6330.875419":>12} 18',
     F['layout']),
    ('an id that ends behind byte 11', f'{7:>14} {"30.875419":>10} {18:>6}', F['layout']),
    ('a fourth token before byte 32', f'{8:>12} {"30.875419":>10} {18:>4} 7 ', F['layout']),
    ('a negative id', f'{-9:>12} {"6330.875419":>12} {18:>6}', F['id']),
    ('a degeneracy with a point', f'{10:>12} {"6330.875419":>12} {"18.0":>6}', F['g']),
]
# forms that the device takes
CLEAN = [
    f'{"+11":>12} {"0.000000":>12} {1:>6}',
    f'{12:>12} {"-.015608":>12} {"+3":>6}',
    f'{13:>12} {"1E22":>12} {0:>6}',
    f'{14:<11} {"5.":<13} {"007":<5}',          # left-justified: energy from byte 12 on
    f'{"000000000015":>12} {"1.5e-21":>12} {999999:>6}',
]


def flagged_record(head, recsize):
    return states_record(None, None, None, recsize, head=head)


def short_line(recsize):
    """A line one byte short and the next line's first byte: a line feed inside the record."""
    rec = states_record(20, '10.500000', 3, recsize)
    return rec[:-2] + b'\n' + b' '


def reference_readings(rec):
    """What the reference's two readings make of a line: (id, energy, g) of `line.split()[0:3]`
    (exomol.py) and (energy, g) of `line[12:32].split()` (partitions.py:407)."""
    tok = rec.split()
    a, b = rec[12:32].split()
    return (int(tok[0]), float(tok[1]), int(tok[2])), (float(a), int(b))


# ---------------------------------------------------------------------------------------------
# Q(T): the exact value and the bound
# ---------------------------------------------------------------------------------------------
TINY = 2.0**-1022
CONTEXT = decimal.Context(prec=50, Emin=-9999999, Emax=9999999)


def exact_q(energy, degeneracy, temps, c2):
    """Q(T) = sum_j g_j exp(-c2 E_j / T) of the same doubles at 50 digits: a list of Decimal."""
    D = decimal.Decimal
    e = [D(float(x)) for x in energy]
    g = [D(float(x)) for x in degeneracy]
    c = D(float(c2))
    out = []
    for t in temps:
        t = D(float(t))
        total = D(0)
        for ej, gj in zip(e, g):
            if gj:
                total = CONTEXT.add(total, CONTEXT.multiply(
                    gj, CONTEXT.exp(CONTEXT.divide(CONTEXT.multiply(-c, ej), t))))
        out.append(total)
    return out


def rel_bound(energy, degeneracy, temps, c2):
    """The relative error any summation order of positive terms may have [ntemp]:
    sum_j w_j (1.5 * 2^-52 * x_j + 1.5 * 2^-52) + (n - 1) * 2^-53 with w_j the term's share of the
    sum and x_j = c2 E_j / T: three roundings in the argument, one ulp of exp and the rounding of
    the product with g; then the additions.  (Evaluated in doubles, relative to the largest term
    so that nothing underflows: the bound is not needed to more than a few digits.)"""
    energy = np.asarray(energy, np.float64)
    g = np.asarray(degeneracy, np.float64)
    n = len(energy)
    out = np.zeros(len(temps))
    for k, t in enumerate(np.asarray(temps, np.float64)):
        x = c2 * energy / t
        live = g > 0
        if not live.any():
            continue
        logw = np.log(g[live]) - x[live]
        w = np.exp(logw - logw.max())
        w /= w.sum()
        out[k] = np.sum(w * (1.5 * 2.0**-52 * x[live] + 1.5 * 2.0**-52)) + (n - 1) * 2.0**-53
    return out


def assert_q(got, exact, bound, n, what=''):
    """got [ntemp] doubles against exact (Decimals) within twice the bound; where the exact sum is
    below n * 2^-1022 only 0 <= got <= n * 2^-1022 is asked."""
    got = np.asarray(got, np.float64)
    assert got.shape == (len(exact),), (what, got.shape)
    for k, (value, want) in enumerate(zip(got, exact)):
        if want < decimal.Decimal(n) * decimal.Decimal(TINY):
            assert 0.0 <= value <= n * TINY, (what, k, value)
            continue
        err = abs((decimal.Decimal(float(value)) - want) / want)
        assert err <= 2 * decimal.Decimal(float(bound[k])), (what, k, float(err), bound[k])


def assert_close(got, other, bound_got, bound_other, n, what=''):
    """Two computed sides of the same sum: their relative difference within the sum of the two
    sides' bounds."""
    got, other = np.asarray(got, np.float64), np.asarray(other, np.float64)
    assert got.shape == other.shape, what
    small = other <= 2 * n * TINY
    assert np.all((got[small] >= 0) & (got[small] <= 2 * n * TINY)), what
    err = np.abs(got[~small] - other[~small]) / other[~small]
    allowed = (np.asarray(bound_got) + np.asarray(bound_other))[~small]
    print(what, 'largest difference over its allowance:',
          float(np.max(err / allowed)) if err.size else 0.0)
    assert np.all(err <= allowed), (what, float(np.max(err / allowed)))


_states_cache = {}


def fixture_states(pf, file):
    """(energy, degeneracy) of a fixture file by the reference's reading, read once."""
    if file not in _states_cache:
        _states_cache[file] = pf.read_states_pf_host(file)
    return _states_cache[file]


_exact_cache = {}
# temperatures at which the fixtures are compared with the exact sum: the ends of both grids
# and 5 K, where x = c2 E / T is about 411 for the lowest NH3 state
EXACT_TEMPS = np.array([5.0, 10.0, 100.0, 300.0, 1500.0, 5000.0])


def fixture_exact(pf, file):
    if file not in _exact_cache:
        e, g = fixture_states(pf, file)
        _exact_cache[file] = exact_q(e, g, EXACT_TEMPS, pf.C2)
    return _exact_cache[file]
