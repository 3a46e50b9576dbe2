"""CPU-only checks of the batched alkali doublets: the C ABI (pb_alkali_voigt_det_batch, the alkali
fields at the end of pb_cont_batch and their checks before any HIP call) and the host side
(Continuum.alkali_species, batch_unsupported(alkali=True), the regime check of the device's
Faddeeva function)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_exported_and_bound():
    from pyratbay_amd import _capi
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pbhip.h')).read(),
                  flags=re.S)
    text = text[:text.index('#ifdef PB_EXPERIMENTS')]
    name = 'pb_alkali_voigt_det_batch'
    assert re.search(r'\b' + name + r'\s*\(', text)
    assert hasattr(_capi.lib(), name)
    assert name in _capi.exported_names()
    for macro, value in (('PB_CONT_MAX_ALKALI', 2), ('PB_CONT_MAX_ALKALI_LINES', 4)):
        assert re.search(rf'#define\s+{macro}\s+{value}\b', text), macro
    # its own argument checks come before any HIP call (fake pointers, never dereferenced)
    fake = C.c_void_p(16)
    wn0 = (C.c_double * 5)(1.0, 2.0, 3.0, 4.0, 5.0)
    with pytest.raises(_capi.PbError, match='at most 4 lines, not 5'):
        _capi.call(name, fake, fake, fake, 30.0, 23.0, 0.07, wn0, 5, 12, 8, None)
    with pytest.raises(_capi.PbError, match='null pointer'):
        _capi.call(name, None, fake, fake, 30.0, 23.0, 0.07, wn0, 2, 12, 8, None)
    assert _capi.call(name, None, None, None, 30.0, 23.0, 0.07, None, 0, 12, 8, None) == 0


def _struct(**kw):
    from pyratbay_amd.continuum import ContBatchStruct
    st = ContBatchStruct()
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def _alkali_struct(nalkali=1, nlines=2, cutoff=4500.0):
    st = _struct(nalkali=nalkali, wn_d=16, alkali_pressure_d=16, alkali_density_d=16)
    for m in range(min(nalkali, 2)):
        st.alkali_nlines[m] = nlines
        st.alkali_cutoff[m] = cutoff
        st.alkali_part_func[m], st.alkali_mass[m] = 2.0, 23.0
    return st


def _call(st, limited=False):
    from pyratbay_amd import _capi
    fake = C.c_void_p(16)          # never dereferenced: the checks come first
    args = [fake] * 6 + [4, 6, 12, 1000, 8, C.byref(st)]
    if limited:
        return _capi.call('pb_interp_ec_batch_cont_limited', *args, None, 0, None, None)
    return _capi.call('pb_interp_ec_batch_cont', *args, None)


@pytest.mark.parametrize('limited', [False, True])
def test_alkali_fields_checked_before_any_hip_call(limited):
    from pyratbay_amd import _capi
    with pytest.raises(_capi.PbError, match='at most 2 alkali models, not 3'):
        _call(_alkali_struct(nalkali=3), limited)
    with pytest.raises(_capi.PbError, match='alkali model 0: 1-4 lines, not 0'):
        _call(_alkali_struct(nlines=0), limited)
    with pytest.raises(_capi.PbError, match='alkali model 0: 1-4 lines, not 9'):
        _call(_alkali_struct(nlines=9), limited)
    with pytest.raises(_capi.PbError, match='at most 4 alkali lines in all, not 6'):
        _call(_alkali_struct(nalkali=2, nlines=3), limited)
    for cutoff in (0.0, -4500.0):
        with pytest.raises(_capi.PbError, match=r'alkali model 0: cutoff \S+ \(must be positive\)'):
            _call(_alkali_struct(cutoff=cutoff), limited)
    st = _alkali_struct()
    st.alkali_density_d = None
    with pytest.raises(_capi.PbError, match='null alkali density'):
        _call(st, limited)
    st = _alkali_struct()
    st.alkali_pressure_d = None
    with pytest.raises(_capi.PbError, match='null alkali pressure'):
        _call(st, limited)
    st = _alkali_struct()
    st.wn_d = None
    with pytest.raises(_capi.PbError, match='null wn'):
        _call(st, limited)


def test_struct_size_and_trailing_fields_round_trip():
    """The alkali fields are appended: the fields before them keep their offsets, and the values
    of the last ones arrive where the library reads them."""
    from pyratbay_amd import _capi
    from pyratbay_amd.continuum import ContBatchStruct
    names = [f[0] for f in ContBatchStruct._fields_]
    first = names.index('nalkali')
    assert names[first - 3:first] == ['pars_d', 'npars', 'pars_stride']
    assert names[first:] == ['nalkali', 'alkali_nlines', 'alkali_wn0', 'alkali_gf',
                             'alkali_detuning', 'alkali_mass', 'alkali_lpar', 'alkali_part_func',
                             'alkali_cutoff', 'alkali_pressure_d', 'alkali_density_d']
    # 4-byte counts, 8-byte doubles and pointers, natural alignment (pbhip.h's declaration)
    assert ContBatchStruct.pars_stride.offset == 604
    assert ContBatchStruct.nalkali.offset == 608
    assert ContBatchStruct.alkali_wn0.offset == 624
    assert ContBatchStruct.alkali_density_d.offset == 840
    assert C.sizeof(ContBatchStruct) == 848
    # the second model's cutoff and partition function, the last doubles of the struct
    st = _alkali_struct(nalkali=2, nlines=2)
    st.alkali_cutoff[1] = -2.5
    with pytest.raises(_capi.PbError, match=r'alkali model 1: cutoff -2\.5 '):
        _call(st)
    st.alkali_cutoff[1] = 4500.0
    st.alkali_part_func[1], st.alkali_mass[1] = -3.0, 39.0
    with pytest.raises(_capi.PbError, match=r'alkali model 1: partition function -3, mass 39'):
        _call(st)
    # the record of a (walker, layer) grows by 6 doubles per alkali line
    lib = _capi.lib()
    base = lib.pb_interp_ec_batch_cont_work_doubles(C.byref(_struct(nrank1=2)), 12, 1000, 8)
    st = _alkali_struct(nalkali=2, nlines=2)
    st.nrank1 = 2
    assert lib.pb_interp_ec_batch_cont_work_doubles(C.byref(st), 12, 1000, 8) == \
        base + 8 * 12 * 6 * 4
    assert lib.pb_interp_ec_batch_cont_work_doubles(C.byref(_alkali_struct(nalkali=3)), 12, 1000,
                                                    8) == -1
    assert lib.pb_interp_ec_batch_cont_work_doubles(C.byref(_alkali_struct(nlines=0)), 12, 1000,
                                                    8) == -1


class _Narrow:
    """A VanderWaals subclass made by a user: a detuning distance of a few Gaussian widths."""

    @staticmethod
    def make(ct, pressure, wn):
        class NarrowVdW(ct.VanderWaals):
            def __init__(self, pressure, wn, cutoff=4500.0):
                self.name, self.species = 'narrow_vdw', 'Na'
                self.wn0, self.gf = [16960.87], [0.65464]
                self.lpar, self.Z, self.detuning, self.mass = 0.071, 2.0, 0.5, 22.989769
                super().__init__(pressure, np.asarray(wn, float), cutoff)
        return NarrowVdW(pressure, wn)


def test_host_side_of_the_alkali_batch():
    from pyratbay_amd import continuum as ct
    wn = np.linspace(8000.0, 22000.0, 50)
    pressure = np.logspace(-6, 2, 7)
    na, k = ct.SodiumVdW(pressure, wn=wn), ct.PotassiumVdW(pressure, wn=wn)
    ray = ct.Kurucz(wn, 'H2')
    cont = ct.Continuum(wn, pressure, [ray, k, na, ct.Deck(pressure, wn)])
    assert cont.alkali_species == ['K', 'Na']               # model order
    assert cont.species == ['H2']                           # unchanged by the alkali models
    assert cont.free_pars == []
    # without arguments: what it returned before (deck and alkali refused)
    assert cont.batch_unsupported() == ['deck', 'potassium_vdw', 'sodium_vdw']
    assert cont.batch_unsupported(deck=True) == ['potassium_vdw', 'sodium_vdw']
    assert cont.batch_unsupported(alkali=True) == ['deck']
    assert cont.batch_unsupported(deck=True, alkali=True) == []
    # a third model (six lines) is beyond the batched form whatever the keyword says
    three = ct.Continuum(wn, pressure, [na, k, ct.SodiumVdW(pressure, wn=wn)])
    assert three.batch_unsupported(alkali=True) == ['sodium_vdw', 'potassium_vdw', 'sodium_vdw']
    assert ct.Continuum(wn, pressure, [ray]).alkali_species == []
    # Re z of the Faddeeva argument: 570 ... 941 for Na, 645 ... 1064 for K over 40 ... 6000 K
    assert na.detuning_x(40.0) == pytest.approx(569.67, abs=0.01)
    assert na.detuning_x(6000.0) == pytest.approx(940.23, abs=0.01)
    assert k.detuning_x(40.0) == pytest.approx(644.53, abs=0.01)
    assert k.detuning_x(6000.0) == pytest.approx(1063.78, abs=0.01)
    assert ct.BATCH_MIN_X == 20.0
    cont.check_alkali_batch(40.0)
    narrow = _Narrow.make(ct, pressure, wn)
    assert narrow.detuning_x(40.0) < 20.0
    with pytest.raises(ValueError, match=r"narrow_vdw.*below 20.*use eval\(\)"):
        ct.Continuum(wn, pressure, [narrow]).check_alkali_batch(40.0)
    # a model on another pressure grid than the Continuum's
    other = ct.SodiumVdW(pressure * 2.0, wn=wn)
    with pytest.raises(ValueError, match='pressure grid'):
        ct.Continuum(wn, pressure, [other]).check_alkali_batch(40.0)
