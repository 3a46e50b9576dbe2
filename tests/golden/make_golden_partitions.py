#!/usr/bin/env python3
"""Fixture G33: what the REFERENCE's partition-function step returns for its bundled mock inputs
(pyratbay/opacity/partitions/partitions.py: exomol_states, exomol_pf, kurucz; io.write_pf).

Build container only (needs /root/reference); same scratch import as make_golden_e2e.py.

    python tests/golden/make_golden_partitions.py

Writes tests/golden/g33_partitions.npz:
  input_<file name>: the bytes of the inputs the reference's programs read (data only), which
  tests/partitions_cases.py writes out under their names: 14N-1H3__MockBYTe.states,
  15N-1H3__MockBYTe-15.states, 1H-12C-14N__MockHarris.states, mock_h2opartfn.dat,
  mock_tiopart.dat, and the `.pf` files this script writes itself (`<T> <Q>` lines from a formula):
  1H-12C-14N__GenA.pf and 1H-13C-14N__GenB.pf of equal length, 1H-12C-15N__GenShort.pf shorter,
  1H-13C-15N__GenShifted.pf shorter and on other temperatures;
  c2: the reference's h c / k;
  states_<nh3|hcn>_<grid>_{pf, temps, isotopes, file}: what exomol_states returned for the NH3 pair
  and the HCN file at the grids `a` = (100, 1500, 100) and `b` = (5, 5000, 5), and the bytes of
  the file it wrote with outfile=;
  kurucz_<h2o|tio>_{pf, temp, isotopes, file}; pf_<equal|unequal>_{pf, temps, isotopes, file},
  pf_unequal_warnings, pf_incompatible_error, mixed_error, molecules_error: the texts of the
  reference's warning and errors.
Only data: arrays the reference returned and bytes it wrote.
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_e2e import reference_package, REF          # noqa: E402

NH3 = ('14N-1H3__MockBYTe.states', '15N-1H3__MockBYTe-15.states')
HCN = ('1H-12C-14N__MockHarris.states',)
KURUCZ = dict(h2o='mock_h2opartfn.dat', tio='mock_tiopart.dat')
GRIDS = dict(a=(100.0, 1500.0, 100.0), b=(5.0, 5000.0, 5.0))


def write_generated_pf(folder):
    """`.pf` files in ExoMol's layout, `%8.1f %15.4f` per line, from a formula of this script."""
    def table(name, temps, scale):
        with open(os.path.join(folder, name), 'w') as f:
            for t in temps:
                f.write(f'{t:8.1f} {scale * t**1.5 + 1.0:15.4f}\n')
    table('1H-12C-14N__GenA.pf', np.arange(1.0, 41.0), 0.25)
    table('1H-13C-14N__GenB.pf', np.arange(1.0, 41.0), 0.50)
    table('1H-12C-15N__GenShort.pf', np.arange(1.0, 31.0), 0.75)
    table('1H-13C-15N__GenShifted.pf', np.arange(1.5, 31.5), 1.00)
    return ('1H-12C-14N__GenA.pf', '1H-13C-14N__GenB.pf', '1H-12C-15N__GenShort.pf',
            '1H-13C-15N__GenShifted.pf')


def main():
    if not os.path.isdir(REF):
        sys.exit('needs /root/reference')
    work = tempfile.mkdtemp(prefix='pb_partitions_')
    try:
        reference_package(work)
        import mc3.utils as mu
        from pyratbay.opacity import partitions
        import pyratbay.constants as pc
        # the import stand-in of mc3's Log keeps its warnings; exomol_pf opens it in a `with`
        logs = []
        mu.Log.__enter__ = lambda self: logs.append(self) or self
        mu.Log.__exit__ = lambda self, *a: False

        inputs = os.path.join(work, 'inputs')
        os.makedirs(inputs)
        for name in NH3 + HCN + tuple(KURUCZ.values()):
            shutil.copy(os.path.join(REF, 'tests', 'inputs', name), inputs)
        generated = write_generated_pf(inputs)
        store = {}
        for name in os.listdir(inputs):
            store['input_' + name] = np.fromfile(os.path.join(inputs, name), np.uint8)
        store['c2'] = pc.h * pc.c / pc.k

        def record(key, got, out, names=('pf', 'isotopes', 'temps')):
            for name, value in zip(names, got):
                store[f'{key}_{name}'] = np.array([str(i) for i in value]) \
                    if name == 'isotopes' else np.asarray(value, float)
            store[f'{key}_file'] = np.fromfile(out, np.uint8)

        out = os.path.join(work, 'out.dat')
        for mol, files in (('nh3', NH3), ('hcn', HCN)):
            for grid, (tmin, tmax, tstep) in GRIDS.items():
                got = partitions.exomol_states([os.path.join(inputs, f) for f in files],
                                               tmin, tmax, tstep, outfile=out)
                record(f'states_{mol}_{grid}', got, out)
        for mol, name in KURUCZ.items():
            got = partitions.kurucz(os.path.join(inputs, name), outfile=out)
            record(f'kurucz_{mol}', got, out, ('pf', 'isotopes', 'temp'))
        a, b, short, shifted = (os.path.join(inputs, f) for f in generated)
        record('pf_equal', partitions.exomol_pf([a, b], outfile=out), out)
        record('pf_unequal', partitions.exomol_pf([a, b, short], outfile=out), out)
        store['pf_unequal_warnings'] = np.array([w for log in logs for w in log.warnings])

        def error_of(call):
            try:
                call()
            except ValueError as e:
                return np.array(str(e))
            raise SystemExit('the reference raised nothing')
        store['pf_incompatible_error'] = error_of(lambda: partitions.exomol_pf([a, shifted]))
        store['mixed_error'] = error_of(
            lambda: partitions.exomol_pf([a, os.path.join(inputs, HCN[0])]))
        store['mixed_states_error'] = error_of(
            lambda: partitions.exomol_states([a, os.path.join(inputs, HCN[0])], 100., 200., 100.))
        store['molecules_error'] = error_of(
            lambda: partitions.exomol_states([os.path.join(inputs, NH3[0]),
                                              os.path.join(inputs, HCN[0])], 100., 200., 100.))
        np.savez_compressed(os.path.join(HERE, 'g33_partitions.npz'), **store)
        for k, v in store.items():
            print(k, np.shape(v))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
