#!/usr/bin/env python3
"""Fixture G29 (tests/golden/g29_isotopes.npz): what the reference makes of an `isotope_ratios`
block (pyratbay/opacity/line_sampling.py:142-238, 282-298, 374-456).  Build container only; the
package is imported as in make_golden_e2e.py:

    python tests/golden/make_golden_isotopes.py

Part A, Line_Sample alone, on small synthetic files written with the reference's writer: three CO
isotopologue files, a second 13CO file that must be ADDED to its slot, and an unlabelled H2O file,
on 4 temperatures x 7 pressures x 33 wavenumbers.  Stored: the files' names and arrays, the
block, the slots (species, isotopes, pnames, pars, iso_ratios, iso_fill, cs_table),
calc_extinction_coefficient(T, dens, pars=...) for several parameter vectors -- a fresh object per
vector, so that no state leaks; the first one with pars=None -- and the error strings of the two
refusals (two keys matching one file, an unknown filler).

Part B, the whole pipeline: pb.run() + eval() from the reference's own
spectrum_{transmission,eclipse}_filters_test.cfg without clouds, alkali and continuum_cross_sec,
with synthetic isotopologue files on the atmosphere's pressures in place of sampled_cross_sec
(the same for both geometries; stored as the table Line_Sample assembles from them), a
narrow window, top-hat bands inside it, an isotope_ratios block and iso_13CO / iso_C18O lines in
retrieval_params.  Stored: the parsed columns, ret.iopacity and map_pars['opacity'] of the
line-sampling model, what the atmosphere is made of, and per parameter vector eval()'s spectrum
and band fluxes with atm.temp, atm.d and atm.radius.  The last vector of a geometry has a negative
filler ratio: it documents what the reference returns there (NaN or a meaningless spectrum, no
reject).  Only data is stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_e2e as e2e                      # noqa: E402
import make_golden_reference_cases as rc           # noqa: E402

REF = e2e.REF
BLOCK = """
    12C-16O 12CO fill_13CO_C18O
    13C-16O 13CO -1.95
    12C-18O C18O -2.7
"""
# (file name, species): the keys of BLOCK are substrings of the names
FILES = [('cs_12C-16O_CO.npz', 'CO'), ('cs_13C-16O_CO_a.npz', 'CO'), ('cs_12C-18O_CO.npz', 'CO'),
         ('cs_H2O.npz', 'H2O'), ('cs_13C-16O_CO_b.npz', 'CO')]
PARS_A = [None, (-0.5, -1.0), (-3.0, -2.0), (-1.0, -0.6), (-0.4, -2.5)]

BANDS = '''# wl  half_width  name
@DATA
1.5025   0.0015   band_a
1.5065   0.0015   band_b
1.5105   0.0015   band_c
'''
#   name          value    pmin    pmax  pstep
RETRIEVAL = """
    log_kappa'     -4.17   -6.0     3.0    0.3
    log_gamma1      0.0    -3.0     3.0    0.3
    log_gamma2      0.0    -3.0     3.0    0.0
    alpha           0.0     0.0     1.0    0.0
    T_irr        1486.0     0.0  3000.0   50.0
    T_int         100.0     0.0  1000.0    0.0
    R_planet        1.05    0.5     4.5    0.03
    M_planet        0.6     0.1     2.0    0.0
    log_H2O        -4.0    -9.0    -1.0    0.5
    iso_13CO       -1.95   -4.0    -0.05   0.3
    iso_C18O       -2.7    -5.0    -0.05   0.3
"""
# (T_irr, R_planet, log_H2O, iso_13CO, iso_C18O); R_planet moves in transit geometry only (the
# eclipse factor of the bands is set once); the last row: a negative filler
VECTORS = [(1486.0, 1.05, -4.0, -1.95, -2.7),
           (1486.0, 1.05, -4.0, -0.5, -1.0),
           (1350.0, 1.02, -3.5, -3.0, -2.0),
           (1600.0, 1.08, -4.5, -1.0, -0.6),
           (1486.0, 1.05, -4.0, -0.4, -2.5),
           (1486.0, 1.05, -4.0, -0.1, -0.2)]


def cross_section(rng, temp, press, nwave):
    base = rng.uniform(-25.0, -19.5, (1, 1, nwave))
    return 10.0**(base + 0.3 * np.log10(press)[None, :, None]
                  + 1.2 * (temp / 2000.0)[:, None, None]
                  + 0.2 * rng.standard_normal((len(temp), len(press), nwave)))


def part_a(store, work):
    import pyratbay.io as io
    import pyratbay.opacity as op
    rng = np.random.default_rng(29)
    temp = np.array([500.0, 1000.0, 1500.0, 2000.0])
    press = np.logspace(-5, 1, 7)
    wn = 4000.0 + 0.5 * np.arange(33)
    folder = os.path.join(work, 'part_a')
    os.makedirs(folder)
    paths = []
    for i, (name, species) in enumerate(FILES):
        cs = cross_section(rng, temp, press, len(wn))
        paths.append(os.path.join(folder, name))
        io.write_opacity(paths[-1], species, temp, press, wn, cs)
        store[f'a_file{i}_cs'] = cs
    store['a_file_names'] = np.array([name for name, _ in FILES])
    store['a_file_species'] = np.array([species for _, species in FILES])
    store['a_temp'], store['a_press'], store['a_wn'] = temp, press, wn
    store['block'] = np.array(BLOCK)
    ls = op.Line_Sample(paths, isotope_ratios=BLOCK)
    store['a_species'] = np.array(ls.species)
    store['a_isotopes'] = np.array(ls.isotopes)
    store['a_pnames'] = np.array(ls.pnames)
    store['a_pars'] = np.array(ls.pars, float)
    store['a_iso_ratios'] = np.array(ls.iso_ratios, float)
    for i, fill in enumerate(ls.iso_fill):
        store[f'a_iso_fill{i}'] = np.array([] if fill is None else fill, np.int64)
    store['a_cs_table'] = ls.cs_table
    layer_temp = np.linspace(650.0, 1850.0, len(press))
    dens = 10.0**rng.uniform(12.0, 16.0, (len(press), ls.nspec))
    store['a_layer_temp'], store['a_dens'] = layer_temp, dens
    store['a_npars'] = np.array(len(PARS_A))
    for k, pars in enumerate(PARS_A):
        fresh = op.Line_Sample(paths, isotope_ratios=BLOCK)
        store[f'a_ec{k}'] = fresh.calc_extinction_coefficient(layer_temp, dens, pars=pars)
        store[f'a_ec{k}_pars'] = np.array(ls.pars if pars is None else pars, float)
        store[f'a_ec{k}_ratios'] = np.array(fresh.iso_ratios, float)
    print('A', list(ls.species), ls.isotopes, ls.pnames, ls.iso_ratios)
    for key, block in (('multiple', BLOCK + '    13C 13CX -2.0\n'),
                       ('filler', BLOCK.replace('fill_13CO_C18O', 'fill_13CO_C17O'))):
        try:
            op.Line_Sample(paths, isotope_ratios=block)
            store[f'a_error_{key}'] = np.array('')
        except ValueError as e:
            # (the message of the first refusal quotes the scratch path: the file name stays)
            store[f'a_error_{key}'] = np.array(str(e).replace(folder + os.sep, ''))
        store[f'a_error_{key}_block'] = np.array(block)
        print('A', key, store[f'a_error_{key}'])


def part_b(store, work, pb):
    import pyratbay.io as io
    import pyratbay.constants as pc
    os.chdir(work)
    with open(os.path.join(work, 'bands.dat'), 'w') as f:
        f.write(BANDS)
    store['b_retrieval_params'] = np.array(RETRIEVAL)
    store['b_vectors'] = np.array(VECTORS)
    store['rjup'], store['mjup'] = np.array(pc.rjup), np.array(pc.mjup)
    for tag in ('transmission', 'eclipse'):
        base = f'{REF}/tests/configs/spectrum_{tag}_filters_test.cfg'
        remove = ['clouds', 'alkali', 'continuum_cross_sec', 'filters']
        reset = {'wl_low': '1.5000 um', 'wl_high': '1.5135 um',
                 'obsfile': os.path.join(work, 'bands.dat')}
        # a first run without tables, for the atmosphere's pressures and the grid
        plain = '\n'.join(line for line in RETRIEVAL.split('\n') if 'iso_' not in line)
        probe = pb.run(rc.make_config(work, base, dict(reset, retrieval_params=plain),
                                      remove + ['sampled_cross_sec'], f'{tag}_probe'))
        press, wn = np.array(probe.atm.press, float), np.array(probe.spec.wn, float)
        # (both geometries share the atmosphere and the window: one set of files, stored once as
        # the table the reference assembles from them -- the files are on the table's own grid)
        rng = np.random.default_rng(2900)
        temp = np.array([500.0, 1200.0, 1900.0, 2600.0])
        folder = os.path.join(work, f'part_b_{tag}')
        os.makedirs(folder)
        paths = []
        for name, species in FILES[:4]:
            paths.append(os.path.join(folder, name))
            io.write_opacity(paths[-1], species, temp, press, wn,
                             cross_section(rng, temp, press, len(wn)))
        store['b_table_temp'] = temp
        reset.update(sampled_cross_sec='\n    ' + '\n    '.join(paths),
                     isotope_ratios=BLOCK, retrieval_params=RETRIEVAL)
        pyrat = pb.run(rc.make_config(work, base, reset, remove, f'{tag}_isotopes'))
        ret, atm, spec, obs = pyrat.ret, pyrat.atm, pyrat.spec, pyrat.obs
        ls = [m for m in pyrat.opacity.models if getattr(m, 'name', '') == 'line sampling'][0]
        j = pyrat.opacity.models.index(ls)
        store[f'{tag}_pnames'] = np.array(ret.pnames)
        for name in ('params', 'pmin', 'pmax', 'pstep', 'prior', 'priorlow', 'priorup'):
            store[f'{tag}_{name}'] = np.array(getattr(ret, name), float)
        store[f'{tag}_iopacity'] = np.array(ret.iopacity[j], np.int64)
        store[f'{tag}_map_opacity'] = np.array(ret.map_pars['opacity'][j], np.int64)
        store[f'{tag}_species'] = np.array(ls.species)
        store[f'{tag}_isotopes'] = np.array(ls.isotopes)
        if 'b_cs_table' in store:
            assert np.array_equal(store['b_cs_table'], ls.cs_table)
        store['b_cs_table'] = ls.cs_table
        store[f'{tag}_wn'] = wn
        store[f'{tag}_rt_path'] = np.array(str(pyrat.od.rt_path))
        # what the atmosphere is made of
        store[f'{tag}_press'] = press
        store[f'{tag}_atm_species'] = np.array(atm.species)
        store[f'{tag}_mol_mass'] = np.array(atm.mol_mass, float)
        store[f'{tag}_base_vmr'] = np.array(atm.base_vmr, float)
        store[f'{tag}_bulk'] = np.array(atm.bulk)
        store[f'{tag}_refpressure'] = np.array(float(atm.refpressure))
        store[f'{tag}_rstar'] = np.array(float(atm.rstar))
        store[f'{tag}_rtop'] = np.array(int(atm.rtop))
        store[f'{tag}_maxdepth'] = np.array(float(pyrat.od.maxdepth))
        store[f'{tag}_runits'] = np.array(str(atm.runits))
        store[f'{tag}_mass_units'] = np.array(str(atm.mass_units))
        store[f'{tag}_nbands'] = np.array(len(obs.filters))
        for i, band in enumerate(obs.filters):
            store[f'{tag}_band{i}_idx'] = np.asarray(band.idx)
            store[f'{tag}_band{i}_response'] = np.asarray(band.response, float)
            store[f'{tag}_band{i}_wl'] = np.asarray(band.wl, float)
            store[f'{tag}_band{i}_height'] = np.array(band.height, float)
            store[f'{tag}_band{i}_photon'] = np.array(band.counting_type != 'energy')
        if tag == 'eclipse':
            store[f'{tag}_quadrature_mu'] = np.array(spec.quadrature_mu, float)
            store[f'{tag}_quadrature_weights'] = np.ravel(spec.quadrature_weights)
            store[f'{tag}_starflux'] = np.array(spec.starflux, float)
            store[f'{tag}_bandflux_star'] = np.array(obs.bandflux_star, float)
        where = {name: i for i, name in enumerate(ret.pnames)}
        rows = {k: [] for k in ('full', 'spectrum', 'bandflux', 'temp', 'dens', 'radius',
                                'rplanet', 'mplanet', 'iso_ratios')}
        for t_irr, r_planet, log_h2o, iso_13co, iso_c18o in VECTORS:
            full = np.array(ret.params, float)
            full[where['T_irr']], full[where['log_H2O']] = t_irr, log_h2o
            if tag == 'transmission':
                full[where['R_planet']] = r_planet
            full[where['iso_13CO']], full[where['iso_C18O']] = iso_13co, iso_c18o
            with np.errstate(all='ignore'):
                spectrum, bandflux = pyrat.eval(full, retmodel=True)
            rows['full'].append(full)
            rows['spectrum'].append(np.array(spectrum, float))
            rows['bandflux'].append(np.array(bandflux, float))
            rows['temp'].append(np.array(atm.temp, float))
            rows['dens'].append(np.array(atm.d, float))
            rows['radius'].append(np.array(atm.radius, float))
            rows['rplanet'].append(float(atm.rplanet))
            rows['mplanet'].append(float(full[where['M_planet']] * pc.mjup))
            rows['iso_ratios'].append(np.array(ls.iso_ratios, float))
            print(tag, full[-2:], 'bandflux', bandflux)
        for k, v in rows.items():
            store[f'{tag}_row_{k}'] = np.array(v)


def main():
    if not os.path.isdir(REF):
        sys.exit('needs /root/reference')
    work = tempfile.mkdtemp(prefix='pb_g29_')
    store = {}
    try:
        pb = e2e.reference_package(work)
        part_a(store, work)
        part_b(store, work, pb)
        out = os.path.join(HERE, 'g29_isotopes.npz')
        np.savez_compressed(out, **store)
        print('g29_isotopes.npz', os.path.getsize(out) // 1024, 'KiB')
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
