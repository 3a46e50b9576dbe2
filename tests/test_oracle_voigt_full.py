"""The oracle's Voigt table (orc.voigt_grid, the plain-C restatement of vprofile.grid) against the
compiled reference (oracle/_ref/vprofile.grid) at the full size of the benchmark configurations:
the GPU tests use the oracle as the independent table at these sizes (test_gpu_voigt.py,
test_gpu_configs.py).  CPU only; runs where the reference extensions were built
(`make -C oracle ref`), about 25 s on one core.

Tolerance: rtol 2e-14 (measured: 4.0e-15) with identical size, index and zero pattern."""
import numpy as np
import pytest

import cases
from oracle import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason='oracle/_ref not built')
RTOL = 2e-14


def reference_rows(vg, dwn):
    vp = ref.module('vprofile')

    def grid(profile, size, index, lorentz, doppler, step):
        assert vp.grid(profile, size, index, lorentz, doppler, step, 0) is not None
    return cases.oracle_voigt_rows(None, vg['lorentz'], vg['doppler'], vg['size'], dwn, grid)


def compare(orc, vg, dwn):
    regimes = cases.voigt_regimes(vg['doppler'], vg['size'], dwn)
    got = reference_rows(vg, dwn)
    want = cases.oracle_voigt_rows(orc, vg['lorentz'], vg['doppler'], vg['size'], dwn)
    return cases.compare_voigt_tables(lambda m, start, n: next(got)[2:], want, regimes, RTOL)


@pytest.mark.parametrize('name', ['c2', 'c3'])
def test_full_size_table_vs_reference(orc, name):
    case = cases.full_width_grid(name)
    worst, count, total = compare(orc, case['voigt'], case['grid']['ownstep'])
    assert all(count.values()), count
    print(f'{name}: {total} samples, cells {count}, worst rel err vs reference '
          + ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))


def test_boundary_grid_vs_reference(orc):
    """The cells on the switches of voigtn (cases.voigt_boundary_case), except the columns one
    ulp below a step/fine switch: the reference is compiled with -ffast-math, which lets the
    compiler turn the divisions of that decision into multiplications by a reciprocal and moves
    the switch by an ulp (the oracle and the HIP planner follow the source in binary64)."""
    c = cases.voigt_boundary_case()
    keep = [n for n in range(len(c['doppler'])) if c['ratio_cols'].get(n, (0, 'at'))[1] == 'at']
    vg = dict(lorentz=c['lorentz'], doppler=c['doppler'][keep], size=c['size'][:, keep])
    worst, count, total = compare(orc, vg, c['dwn'])
    assert all(count.values()), count
    print(f'boundary grid: {total} samples, worst rel err vs reference {worst}')
