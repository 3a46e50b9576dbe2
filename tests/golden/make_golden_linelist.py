#!/usr/bin/env python3
"""Fixture G32: what the REFERENCE's line-list readers return for its bundled mock inputs
(pyratbay/opacity/linelist/{hitran,exomol}.py, `runmode = tli` of opacity/lread.py).

Build container only (needs /root/reference); same scratch import as make_golden_e2e.py.

    python tests/golden/make_golden_linelist.py

Writes tests/golden/g32_linelist.npz:
  input_<file name>: the bytes of the inputs the reference's programs read (data only), which
  tests/linelist_cases.py writes out under their names: Mock_HITRAN_H2O_1.00-1.01um.par,
  14N-1H3__MockBYTe__04999-05000.trans + .states, 15N-1H3__MockBYTe-15__04999-05000.trans +
  .states, PF_Exomol_NH3.dat;
  <input>_recsize, _nrec, _windows [nwin, 2] (make_golden_tli.windows of the full read), and for
  every window k: <input>_w<k>_none (dbread returned None), else _istart, _istop and the four
  arrays _wn, _gf, _elow, _iso that dbread returned;
  h2o_isotopes / _mass / _ratio, nh3_isotopes / _mass / _ratio: the isotope data the readers
  used; h2o_pf_temp, h2o_pf, h2o_pf_isotopes: the TIPS table of H2O;
  nh3_tli: the bytes of the TLI file the reference writes for the two NH3 files together,
  nh3_tli_wl: its wl_low, wl_high in um.
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
from make_golden_tli import windows                          # noqa: E402

INPUTS = dict(
    h2o='Mock_HITRAN_H2O_1.00-1.01um.par',
    nh3_14='14N-1H3__MockBYTe__04999-05000.trans',
    nh3_15='15N-1H3__MockBYTe-15__04999-05000.trans',
)
EXTRA = ('14N-1H3__MockBYTe.states', '15N-1H3__MockBYTe-15.states', 'PF_Exomol_NH3.dat')
NH3_WL = (1.9, 2.1)

CFG_NH3 = '''
[pyrat]
runmode = tli
logfile = {work}/nh3.log
tlifile = {work}/nh3.tli
dblist = {ref}/tests/inputs/{nh3_14}
    {ref}/tests/inputs/{nh3_15}
dbtype = exomol exomol
pflist = {ref}/tests/inputs/PF_Exomol_NH3.dat
wl_low = {lo} um
wl_high = {hi} um
verb = 0
'''


def main():
    if not os.path.isdir(REF):
        sys.exit('needs /root/reference')
    work = tempfile.mkdtemp(prefix='pb_linelist_')
    try:
        pb = reference_package(work)
        import mc3.utils as mu
        from pyratbay.opacity import linelist
        from pyratbay.opacity import partitions
        inputs = os.path.join(REF, 'tests', 'inputs')
        store = {}
        for name in list(INPUTS.values()) + list(EXTRA):
            store['input_' + name] = np.fromfile(os.path.join(inputs, name), np.uint8)
        pffile = os.path.join(inputs, 'PF_Exomol_NH3.dat')
        for key, name in INPUTS.items():
            path = os.path.join(inputs, name)
            reader = linelist.Hitran if key == 'h2o' else linelist.Exomol
            db = reader(path, 'tips' if key == 'h2o' else pffile, mu.Log(verb=0))
            full = db.dbread(-np.inf, np.inf, 0)
            store[f'{key}_recsize'] = db.recsize
            nrec = os.path.getsize(path) // db.recsize
            store[f'{key}_nrec'] = nrec
            wins = windows(full[0])
            store[f'{key}_windows'] = np.array(wins)
            for k, (a, b) in enumerate(wins):
                got = db.dbread(a, b, 0)
                store[f'{key}_w{k}_none'] = got is None
                if got is None:
                    continue
                with open(path, 'r') as data:
                    istart = db.binsearch(data, a, 0, nrec - 1, False)
                    istop = db.binsearch(data, b, istart, nrec - 1, True)
                store[f'{key}_w{k}_istart'], store[f'{key}_w{k}_istop'] = istart, istop
                for col, arr in zip(('wn', 'gf', 'elow', 'iso'), got):
                    store[f'{key}_w{k}_{col}'] = np.asarray(arr)
            mol = 'h2o' if key == 'h2o' else 'nh3'
            store[f'{mol}_isotopes'] = np.array([str(i) for i in db.isotopes])
            store[f'{mol}_mass'] = np.asarray(db.mass, float)
            store[f'{mol}_ratio'] = np.asarray(db.isoratio, float)
            print(key, 'recsize', db.recsize, 'records', nrec, 'lines', len(full[0]))
        pf, iso, temp = partitions.tips('H2O')
        store['h2o_pf_temp'], store['h2o_pf'] = np.asarray(temp, float), np.asarray(pf, float)
        store['h2o_pf_isotopes'] = np.array([str(i) for i in iso])

        cfg = os.path.join(work, 'nh3.cfg')
        with open(cfg, 'w') as f:
            f.write(CFG_NH3.format(work=work, ref=REF, lo=NH3_WL[0], hi=NH3_WL[1],
                                   nh3_14=INPUTS['nh3_14'], nh3_15=INPUTS['nh3_15']))
        pb.run(cfg)
        store['nh3_tli'] = np.fromfile(os.path.join(work, 'nh3.tli'), np.uint8)
        store['nh3_tli_wl'] = np.array(NH3_WL)
        np.savez_compressed(os.path.join(HERE, 'g32_linelist.npz'), **store)
        print('nh3 tli bytes', len(store['nh3_tli']))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
