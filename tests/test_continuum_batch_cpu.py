"""CPU-only checks of the batched continuum's C ABI (pb_interp_ec_batch_cont[_limited],
pb_interp_ec_batch_cont_work_doubles): declared, exported, bound, and their arguments are checked
before any HIP call -- no GPU needed for the errors."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pb_interp_ec_batch_cont', 'pb_interp_ec_batch_cont_limited',
         'pb_interp_ec_batch_cont_work_doubles')


def test_entry_points_declared_exported_and_bound():
    from pyratbay_amd import _capi
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pbhip.h')).read(),
                  flags=re.S)
    text = text[:text.index('#ifdef PB_EXPERIMENTS')]
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert hasattr(_capi.lib(), name)
        assert name in _capi.exported_names()
    assert 'typedef struct pb_cont_batch' in text


def _struct(**kw):
    from pyratbay_amd.continuum import ContBatchStruct
    st = ContBatchStruct()
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def _call(st, limited=False):
    from pyratbay_amd import _capi
    fake = C.c_void_p(16)          # never dereferenced: the checks come first
    args = [fake] * 6 + [4, 6, 12, 1000, 8, None if st is None else C.byref(st)]
    if limited:
        return _capi.call('pb_interp_ec_batch_cont_limited', *args, None, 0, None, None)
    return _capi.call('pb_interp_ec_batch_cont', *args, None)


@pytest.mark.parametrize('limited', [False, True])
def test_argument_checks_before_any_hip_call(limited):
    from pyratbay_amd import _capi
    with pytest.raises(_capi.PbError, match='null continuum'):
        _call(None, limited)
    with pytest.raises(_capi.PbError, match='at most 4 CIA tables, not 5'):
        _call(_struct(ncia=5), limited)
    with pytest.raises(_capi.PbError, match='at most one H- model, not 2'):
        _call(_struct(hminus=2), limited)
    with pytest.raises(_capi.PbError, match='rank-1 models, not 9'):
        _call(_struct(nrank1=9), limited)
    # the counts at the end of the struct come through (its layout matches pbhip.h)
    with pytest.raises(_capi.PbError, match=r'ncs 3, npars 5, pars_stride 7'):
        _call(_struct(ncs=3, npars=5, pars_stride=7), limited)
    # a Rayleigh term without its cross section; with it, a species index out of range
    st = _struct(nrank1=1, ncs=2)
    with pytest.raises(_capi.PbError, match='null cross section'):
        _call(st, limited)
    st.rank1_cs_d[0] = 16
    st.rank1_species[0] = 2
    with pytest.raises(_capi.PbError, match='species 2 of 2'):
        _call(st, limited)
    # a CIA table without arrays, then with too few temperatures
    st = _struct(ncia=1, ncs=2)
    with pytest.raises(_capi.PbError, match='null CIA table'):
        _call(st, limited)
    st.cia_tab_d[0] = st.cia_temps_d[0] = 16
    st.cia_ntemp[0] = 1
    with pytest.raises(_capi.PbError, match='1 temperatures'):
        _call(st, limited)
    # Lecavelier parameters beyond npars; H- without its arrays; no density
    st = _struct(nrank1=1, npars=1, ncs=1)
    st.rank1_kind[0], st.rank1_pressure_d[0] = 1, 16
    with pytest.raises(_capi.PbError, match='parameters 0.. of 1'):
        _call(st, limited)
    with pytest.raises(_capi.PbError, match='null H- arrays'):
        _call(_struct(hminus=1, ncs=2), limited)
    st = _struct(nrank1=1, ncs=1)
    st.rank1_cs_d[0] = 16
    with pytest.raises(_capi.PbError, match='null continuum density'):
        _call(st, limited)
    assert b'null continuum density' in _capi.lib().pb_last_error()


def test_work_doubles():
    from pyratbay_amd import _capi
    lib = _capi.lib()
    assert lib.pb_interp_ec_batch_cont_work_doubles(None, 12, 1000, 8) == -1
    assert lib.pb_interp_ec_batch_cont_work_doubles(C.byref(_struct(ncia=5)), 12, 1000, 8) == -1
    # the interpolation's own scratch + one record per (walker, layer) + the Lecavelier rows
    st = _struct(nrank1=2, ncia=2, hminus=1)
    st.rank1_kind[1] = 1
    n = 8 * 12
    got = lib.pb_interp_ec_batch_cont_work_doubles(C.byref(st), 12, 1000, 8)
    assert got >= n * 16 + n // 2 + n * (2 + 4 * 2 + 10) + 8 * 1000
