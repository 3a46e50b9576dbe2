"""The partition-function step on the host (pyratbay_amd/partitions.py with device=False, exomol_pf,
kurucz, write_pf) against what the reference returned and wrote (g33_partitions.npz), the host
statement of the states parse against int() / float(), and Q(T) against exact arithmetic."""
import os

import numpy as np
import pytest

import partitions_cases as pc
from pyratbay_amd import linelist as ll
from pyratbay_amd import partitions as pf


def _golden(key):
    g = pc.g33()
    return {name: g[f'{key}_{name}'] for name in ('pf', 'isotopes', 'file')}


def _file_bytes(path):
    with open(path, 'rb') as f:
        return f.read()


def test_c2_and_the_grids_have_the_references_bits():
    g = pc.g33()
    assert pc.bits(pf.C2) == pc.bits(g['c2'])
    for mol in ('nh3', 'hcn'):
        for grid, args in pc.GRIDS.items():
            temps = pf.temperature_grid(*args)
            assert np.array_equal(pc.bits(temps), pc.bits(g[f'states_{mol}_{grid}_temps']))
    assert len(pf.temperature_grid(5.0, 5000.0, 5.0)) == 1000


@pytest.mark.parametrize('mol', ['nh3', 'hcn'])
@pytest.mark.parametrize('grid', ['a', 'b'])
def test_exomol_states_host_route(mol, grid, tmp_path, capsys):
    """The arrays within the summed bounds of the two sides (both are NumPy's exp and sum, of two
    builds), the grid bit for bit, the names, and the written file byte for byte."""
    want = _golden(f'states_{mol}_{grid}')
    out = str(tmp_path / 'PF.dat')
    q, isotopes, temps = pf.exomol_states(pc.STATES[mol], *pc.GRIDS[grid], outfile=out,
                                          device=False)
    assert np.array_equal(pc.bits(temps), pc.bits(pc.g33()[f'states_{mol}_{grid}_temps']))
    assert isotopes == list(want['isotopes']) and q.shape == want['pf'].shape
    for i, file in enumerate(pc.STATES[mol]):
        e, g = pc.fixture_states(pf, file)
        bound = pc.rel_bound(e, g, temps, pf.C2)
        pc.assert_close(q[i], want['pf'][i], bound, bound, len(e), file)
    assert _file_bytes(out) == want['file'].tobytes()
    text = capsys.readouterr().out
    assert f"for molecule {mol.upper()}, with isotopes {isotopes}" in text
    assert f'temperature range {temps[0]:.0f}--{temps[-1]:.0f} K.' in text


def test_exomol_states_default_outfile_and_string_argument(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    q, isotopes, temps = pf.exomol_states(pc.HCN[0], 100.0, 1500.0, 100.0, outfile='default',
                                          device=False)
    assert _file_bytes('PF_exomol_HCN.dat') == pc.g33()['states_hcn_a_file'].tobytes()
    # what was written reads back as a partition of make_tli
    back, iso, t = ll.read_pf('PF_exomol_HCN.dat')
    assert iso == isotopes and np.array_equal(t, temps)
    np.testing.assert_allclose(back, q, rtol=1e-7)


@pytest.mark.parametrize('file', pc.NH3 + pc.HCN)
def test_host_statement_against_exact_arithmetic(file):
    """The reference's own statement within twice the bound of the 50-digit sum, at 5 K (x about
    411 for the lowest NH3 state) as at 5000 K; and the golden arrays within their bound."""
    e, g = pc.fixture_states(pf, file)
    exact = pc.fixture_exact(pf, file)
    bound = pc.rel_bound(e, g, pc.EXACT_TEMPS, pf.C2)
    pc.assert_q(pf.states_partition_host(e, g, pc.EXACT_TEMPS), exact, bound, len(e), file)
    mol, i = ('hcn', 0) if file in pc.HCN else ('nh3', pc.NH3.index(file))
    g33 = pc.g33()
    temps = g33[f'states_{mol}_b_temps']
    at = [int(np.nonzero(temps == t)[0][0]) for t in pc.EXACT_TEMPS]
    pc.assert_q(g33[f'states_{mol}_b_pf'][i, at], exact, bound, len(e), file)


def test_bound_and_exact_sum_on_a_case_with_known_values():
    """Two states, E = 0 and E = T / c2: Q = g0 + g1 / e."""
    t = 250.0
    energy = np.array([0.0, t / pf.C2])
    exact = pc.exact_q(energy, [3, 5], [t], pf.C2)[0]
    assert abs(float(exact) - (3 + 5 * np.exp(-1.0))) < 1e-13
    bound = pc.rel_bound(energy, [3, 5], [t], pf.C2)[0]
    assert 1.5 * 2.0**-52 < bound < 4 * 2.0**-52
    pc.assert_q(pf.states_partition_host(energy, np.array([3, 5]), [t]), [exact], [bound], 2)
    with pytest.raises(AssertionError):
        pc.assert_q([float(exact) * (1 + 1e-14)], [exact], [bound], 2)
    # every term underflows: only the range is asked
    cold = pc.exact_q([1e4, 2e4], [3, 5], [1.0], pf.C2)
    assert 0 < cold[0] < pc.TINY
    pc.assert_q([0.0], cold, [1.0], 2)
    with pytest.raises(AssertionError):
        pc.assert_q([1e-300], cold, [1.0], 2)


@pytest.mark.parametrize('mol', ['h2o', 'tio'])
def test_kurucz(mol, tmp_path):
    g = pc.g33()
    out = str(tmp_path / 'PF.dat')
    q, isotopes, temp = pf.kurucz(pc.KURUCZ[mol], outfile=out)
    assert np.array_equal(pc.bits(q), pc.bits(g[f'kurucz_{mol}_pf']))
    assert np.array_equal(pc.bits(temp), pc.bits(g[f'kurucz_{mol}_temp']))
    assert isotopes == list(g[f'kurucz_{mol}_isotopes'])
    assert _file_bytes(out) == g[f'kurucz_{mol}_file'].tobytes()
    with pytest.raises(ValueError, match='Invalid Kurucz partition-function file.'):
        pf.kurucz('other.dat')


def test_exomol_pf_equal_unequal_incompatible(tmp_path):
    g = pc.g33()
    out = str(tmp_path / 'PF.dat')
    for key, files in (('pf_equal', [pc.PF_A, pc.PF_B]),
                       ('pf_unequal', [pc.PF_A, pc.PF_B, pc.PF_SHORT])):
        if key == 'pf_unequal':
            with pytest.warns(UserWarning) as caught:
                q, isotopes, temps = pf.exomol_pf(files, outfile=out)
            assert [str(w.message) for w in caught] == list(g['pf_unequal_warnings'])
        else:
            q, isotopes, temps = pf.exomol_pf(files, outfile=out)
        assert np.array_equal(pc.bits(q), pc.bits(g[f'{key}_pf']))
        assert np.array_equal(pc.bits(temps), pc.bits(g[f'{key}_temps']))
        assert isotopes == list(g[f'{key}_isotopes'])
        assert _file_bytes(out) == g[f'{key}_file'].tobytes()
    with pytest.raises(ValueError) as err:
        pf.exomol_pf([pc.PF_A, pc.PF_SHIFTED])
    assert str(err.value) == str(g['pf_incompatible_error'])
    one, isotopes, _ = pf.exomol_pf(pc.PF_A)
    assert one.shape == (1, 40) and isotopes == ['124']


def test_the_references_error_texts():
    g = pc.g33()
    with pytest.raises(ValueError) as err:
        pf.exomol_pf([pc.PF_A, pc.HCN[0]])
    assert str(err.value) == str(g['mixed_error'])
    with pytest.raises(ValueError) as err:
        pf.exomol_states([pc.PF_A, pc.HCN[0]], 100.0, 200.0, 100.0, device=False)
    assert str(err.value) == str(g['mixed_states_error'])
    with pytest.raises(ValueError) as err:
        pf.exomol_states([pc.NH3[0], pc.HCN[0]], 100.0, 200.0, 100.0, device=False)
    assert str(err.value) == str(g['molecules_error'])
    assert pf.check_exomol_files(pc.NH3) == ('states', 'NH3', ['4111', '5111'])
    assert pf.check_exomol_files([pc.PF_A, pc.PF_B]) == ('pf', 'HCN', ['124', '134'])
    assert pf.check_exomol_files([pc.PF_A, pc.HCN[0]])[0] == ''
    assert pf.check_exomol_files(['x/1H-12C-14N__Harris.states.bz2'])[0] == 'states'
    with pytest.raises(ValueError, match='TIPS 2021 table .* is not shipped'):
        pf.tips('H2O')
    with pytest.raises(ValueError, match='does not match with the number of isotopes'):
        pf.write_pf(os.devnull, np.zeros((2, 3)), ['a'], np.zeros(3))
    with pytest.raises(ValueError, match='does not match with the number of temperature'):
        pf.write_pf(os.devnull, np.zeros((2, 3)), ['a', 'b'], np.zeros(4))


def test_bz2_states_give_the_same_arrays(tmp_path):
    import bz2
    packed = str(tmp_path / os.path.basename(pc.HCN[0])) + '.bz2'
    with bz2.open(packed, 'wb') as f:
        f.write(_file_bytes(pc.HCN[0]))
    q, isotopes, _ = pf.exomol_states(packed, 100.0, 1500.0, 100.0, device=False)
    plain = pf.exomol_states(pc.HCN[0], 100.0, 1500.0, 100.0, device=False)[0]
    assert np.array_equal(pc.bits(q), pc.bits(plain)) and isotopes == ['124']


# ---------------------------------------------------------------------------------------------
# the host statement of the states parse
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('file', pc.NH3 + pc.HCN)
def test_parse_statement_agrees_with_int_and_float_on_the_fixtures(file):
    data = _file_bytes(file)
    recsize = pc.RECSIZE[file]
    assert len(data) % recsize == 0
    ids, energy, g, flags = pf.parse_states_host(data, recsize)
    assert not flags.any() and len(ids) == len(data) // recsize
    lines = data.splitlines(keepends=True)
    assert len(lines) == len(ids)
    for i, line in enumerate(lines):
        (want_id, want_e, want_g), (pf_e, pf_g) = pc.reference_readings(line)
        assert ids[i] == want_id and g[i] == want_g == pf_g
        assert pc.bits(energy[i]) == pc.bits(want_e) == pc.bits(pf_e)
    # and with the two readers built on those readings
    e_pf, g_pf = pf.read_states_pf_host(file)
    assert np.array_equal(pc.bits(e_pf), pc.bits(energy)) and np.array_equal(g_pf, g)
    dense_e, dense_g = ll.read_states(file)
    assert np.array_equal(pc.bits(dense_e[ids]), pc.bits(energy))
    assert np.array_equal(dense_g[ids], g)


@pytest.mark.parametrize('recsize', [33, 86, 139, 255])
def test_parse_statement_flags_exactly_the_constructed_records(recsize):
    rng = np.random.default_rng(33)
    records = [pc.random_states(rng, 1, recsize, first_id=100 + i) for i in range(40)]
    want = np.zeros(40, np.uint8)
    for k, (what, head, bits) in enumerate(pc.FLAGGED):
        records[2 * k + 1] = pc.flagged_record(head, recsize)
        want[2 * k + 1] = bits
    records[29] = pc.short_line(recsize)
    want[29] = pc.F['layout']
    for k, head in enumerate(pc.CLEAN):
        records[30 + k] = pc.flagged_record(head, recsize)
    ids, energy, g, flags = pf.parse_states_host(b''.join(records), recsize)
    assert np.array_equal(flags != 0, want != 0)
    if recsize > 36:
        assert np.array_equal(flags, want)
    # a flagged token is -1 / NaN; every clean record is what both readings of the reference give
    whole = (flags & (pc.F['token'] | pc.F['layout'])) != 0
    assert np.all(ids[whole | (flags & pc.F['id'] != 0)] == -1)
    assert np.all(np.isnan(energy[whole | (flags & pc.F['energy'] != 0)]))
    assert np.all(np.isnan(g[whole | (flags & pc.F['g'] != 0)]))
    for i in np.nonzero(flags == 0)[0]:
        (want_id, want_e, want_g), (pf_e, pf_g) = pc.reference_readings(records[i])
        assert ids[i] == want_id and g[i] == want_g == pf_g
        assert pc.bits(energy[i]) == pc.bits(want_e) == pc.bits(pf_e)
    # the energy rule is the line-list kernels' rule
    for text in ('6330.875419', '1.5e+24', 'NaN', '1_000.5', '1E22', '-0.0', '1.2.3'):
        value, flagged = ll.decimal_fast_path_host(text)
        rec = pc.states_record(1, text, 18, recsize)
        got = pf.states_record_host(rec, recsize)
        assert (got[3] == pc.F['energy']) == flagged
        assert pc.same_columns([got[1]], [value])


def test_flag_bits_and_sizes_are_the_headers():
    from pyratbay_amd import _capi
    for name, bit in pf.STATES_FLAGS.items():
        assert _capi.constant('PB_LL_STATES_' + name.upper()) == bit == pc.F[name]
    protos = _capi.header().protos
    assert {'pb_parse_states', 'pb_pf_states', 'pb_pf_states_work'} <= set(protos)
    assert _capi.constant('PB_PF_TEMPS_PER_TILE') == 1024
    assert _capi.constant('PB_STATES_RECORDS_PER_BLOCK') == 128
