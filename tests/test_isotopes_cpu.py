"""The isotope ratios of sampled cross sections on the host (pyratbay_amd/isotopes.py: the NumPy
specification of pb_iso_density) against fixture G29 part A, which comes from the reference's
Line_Sample itself (tests/golden/make_golden_isotopes.py)."""
import numpy as np
import pytest

from pyratbay_amd import isotopes as iso
from pyratbay_amd.atmosphere import MAX_ISO_FILLERS, MAX_ISO_SLOTS, REJECT_ISOTOPE


def bits(a):
    return np.ascontiguousarray(a, float).view(np.int64)


def model_of(g, block=None):
    entries = iso.parse(str(g['block']) if block is None else block)
    names = [str(n) for n in g['a_file_names']]
    species, labels, index = iso.assign(entries, names, [str(s) for s in g['a_file_species']])
    return iso.IsotopeRatios(species, labels, entries), index


def test_slots_and_defaults_equal_the_reference(golden):
    g = golden('g29_isotopes')
    entries = iso.parse(str(g['block']))
    assert entries == [('12C-16O', 'iso_12CO', 'fill_13CO_C18O'), ('13C-16O', 'iso_13CO', '-1.95'),
                       ('12C-18O', 'iso_C18O', '-2.7')]
    model, index = model_of(g)
    assert list(model.species) == [str(s) for s in g['a_species']] == ['CO', 'CO', 'CO', 'H2O']
    assert model.isotopes == [str(s) for s in g['a_isotopes']]
    assert model.pnames == [str(s) for s in g['a_pnames']] == ['iso_13CO', 'iso_C18O']
    assert np.array_equal(model.pars, g['a_pars']) and model.npars == 2
    for i in range(model.nspec):
        fill = [int(j) for j in g[f'a_iso_fill{i}']]
        assert (model.iso_fill[i] or []) == fill
    # the second 13CO file goes to the slot of the first
    assert index == [0, 1, 2, 3, 1]
    # the host statement is the reference's arithmetic: equal bits
    assert np.array_equal(bits(model.iso_ratios), bits(g['a_iso_ratios']))
    assert list(model.kind) == [iso.KIND_FILL, iso.KIND_FREE, iso.KIND_FREE, iso.KIND_CONST]
    assert list(model.par_column) == [-1, 0, 1, -1]
    for k in range(int(g['a_npars'])):
        got = model.ratios_host(g[f'a_ec{k}_pars'][None])[0]
        assert np.array_equal(bits(got), bits(g[f'a_ec{k}_ratios'])), k
        assert got[3] == 1.0


def test_refusals_of_the_reference(golden):
    g = golden('g29_isotopes')
    assert str(g['a_error_multiple']) == "Multiple isotope labels match 'cs_13C-16O_CO_a.npz'"
    assert str(g['a_error_filler']) == 'Invalid filler'
    with pytest.raises(ValueError) as e:
        model_of(g, str(g['a_error_multiple_block']))
    assert str(e.value) == str(g['a_error_multiple'])
    with pytest.raises(ValueError) as e:
        model_of(g, str(g['a_error_filler_block']))
    assert str(e.value) == str(g['a_error_filler'])
    # an unlabelled file keeps the rule of a load without a block
    entries = iso.parse(str(g['block']))
    species, labels, index = iso.assign(entries, ['a_H2O.npz', 'b_H2O.npz', 'c_CH4.npz'],
                                        ['H2O', 'H2O', 'CH4'])
    assert (species, labels, index) == (['H2O', 'CH4'], ['', ''], [0, 0, 1])


def test_extinction_equals_the_reference(golden, orc):
    """interp_ec on dens * ratios_host(pars) against the reference's
    calc_extinction_coefficient(T, dens, pars=pars) of a fresh object, at the tolerance
    test_line_sample.py has for the chain behind interp_ec (1e-10)."""
    g = golden('g29_isotopes')
    model, _ = model_of(g)
    temp, dens, table = g['a_layer_temp'], g['a_dens'], g['a_cs_table']
    nlayers, nwave = len(temp), table.shape[3]
    for k in range(int(g['a_npars'])):
        ratios = model.ratios_host(g[f'a_ec{k}_pars'][None])[0]
        ec = np.zeros((nlayers, nwave))
        orc.interp_ec(ec, table, g['a_temp'], temp, np.ascontiguousarray(dens * ratios), 0,
                      nlayers)
        want = g[f'a_ec{k}']
        print(f'pars {g[f"a_ec{k}_pars"]}: max rel err {np.max(np.abs(ec / want - 1)):.2e}')
        np.testing.assert_allclose(ec, want, rtol=1e-10)
    # the ratios matter: the defaults' result is not another vector's
    assert np.max(np.abs(g['a_ec1'] / g['a_ec0'] - 1)) > 1e-3


def test_deviations_are_refused():
    species, labels = ['CO'] * 3, ['iso_a', 'iso_b', 'iso_c']
    with pytest.raises(ValueError, match='is a fill slot itself'):
        iso.IsotopeRatios(species, labels, [('a', 'iso_a', 'fill_b_c'), ('b', 'iso_b', 'fill_c'),
                                            ('c', 'iso_c', '-2.0')])
    n = MAX_ISO_FILLERS + 1
    names = [f'iso_f{k}' for k in range(n)]
    entries = [(f'k{k}', name, '-3.0') for k, name in enumerate(names)]
    fill = 'fill_' + '_'.join(f'f{k}' for k in range(n))
    with pytest.raises(ValueError, match=f'{n} fillers: at most {MAX_ISO_FILLERS}'):
        iso.IsotopeRatios(['CO'] * (n + 1), ['iso_main'] + names,
                          [('m', 'iso_main', fill)] + entries)
    ok = iso.IsotopeRatios(['CO'] * n, ['iso_main'] + names[:-1],
                           [('m', 'iso_main', fill.rsplit('_', 1)[0])] + entries[:-1])
    assert len(ok.iso_fill[0]) == MAX_ISO_FILLERS
    many = MAX_ISO_SLOTS + 1
    with pytest.raises(ValueError, match=f'{many} labelled isotope slots: at most {MAX_ISO_SLOTS}'):
        iso.IsotopeRatios(['CO'] * many, [f'iso_s{k}' for k in range(many)],
                          [(f'k{k}', f'iso_s{k}', '-2.0') for k in range(many)])
    with pytest.raises(ValueError, match='key label ratio'):
        iso.parse('13C 13CO')
    with pytest.raises(ValueError):
        iso.parse('13C 13CO minus_two')


def test_scale_host_reject_contract(golden):
    g = golden('g29_isotopes')
    model, _ = model_of(g)
    rng = np.random.default_rng(5)
    nw, nlayers = 6, 3
    temps = rng.uniform(800.0, 1500.0, (nw, nlayers))
    dens = rng.uniform(1e10, 1e14, (nw, nlayers, model.nspec))
    pars = np.tile(model.pars, (nw, 1))
    pars[1] = (-0.1, -0.2)                      # the filler goes negative
    pars[2, 1] = np.nan
    pars[4, 0] = np.inf
    pars[5, 0] = -np.inf                        # a ratio of exactly 0 is a ratio
    ratios = model.ratios_host(pars)
    assert ratios[1, 0] < 0 and np.isnan(ratios[2, 2]) and ratios[5, 1] == 0.0
    t, d, reject = model.scale_host(temps, dens, pars)
    bad = [1, 2, 4]
    assert list(np.flatnonzero(reject)) == bad and np.all(reject[bad] == REJECT_ISOTOPE)
    assert reject.dtype == np.int32 and REJECT_ISOTOPE == 32
    assert np.all(t[bad] == 0.0) and np.all(d[bad] == 0.0)
    good = [0, 3, 5]
    assert np.array_equal(t[good], temps[good])
    assert np.array_equal(bits(d[good]), bits(dens[good] * ratios[good][:, None, :]))
    assert np.array_equal(bits(d[0][:, 3]), bits(dens[0][:, 3]))         # unlabelled: untouched
    # None: the defaults, with the reference's bits
    t0, d0, r0 = model.scale_host(temps, dens)
    assert not np.any(r0) and np.array_equal(bits(d0), bits(dens * g['a_iso_ratios']))
    with pytest.raises(ValueError, match=r'iso_pars must have shape \(nw, 2\)'):
        model.scale_host(temps, dens, pars[:, :1])
