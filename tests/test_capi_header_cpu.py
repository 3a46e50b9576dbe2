"""The binding reads its constants, struct layouts and prototypes from include/pbhip.h
(_capi.parse_header): the layouts against the C compiler's, prototypes of every type class against
a frozen copy, the reader's refusals, one read per process, and which entries call() checks."""
import builtins
import ctypes as C
import os
import re
import subprocess

import pytest

from pyratbay_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = ('pb_radeq', 'pb_radeq_convection', 'pb_cont_batch', 'pb_cloud_terms', 'pb_cloud_models',
           'pb_atm_model', 'pb_chem_model', 'pb_iso_model')


def test_layout_and_constants_against_the_compiler(tmp_path):
    """sizeof of every struct, offsetof and sizeof of every field and the value of every constant,
    as a C compiler reads the header, equal what the reader derived."""
    hdr = _capi.header()
    assert set(hdr.structs) >= set(STRUCTS) and len(hdr.constants) >= 40
    lines, derived = [], {}
    for tag, cls in hdr.structs.items():
        lines.append(f'printf("sizeof {tag} %zu\\n", sizeof({tag}));')
        derived[f'sizeof {tag}'] = C.sizeof(cls)
        for name, _ in cls._fields_:
            lines.append(f'printf("field {tag}.{name} %zu %zu\\n", offsetof({tag}, {name}), '
                         f'sizeof((({tag} *)0)->{name}));')
            field = getattr(cls, name)
            derived[f'field {tag}.{name}'] = (field.offset, field.size)
    for name, value in hdr.constants.items():
        lines.append(f'printf("constant {name} %lld\\n", (long long)({name}));')
        derived[f'constant {name}'] = value
    source = tmp_path / 'layout.c'
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbhip.h"\n'
                      'int main(void) {\n' + '\n'.join(lines) + '\nreturn 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC') or 'cc', '-I', os.path.join(ROOT, 'include'),
                    str(source), '-o', str(exe)], check=True)
    compiled = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        kind, name, *numbers = line.split()
        numbers = tuple(map(int, numbers))
        compiled[f'{kind} {name}'] = numbers if kind == 'field' else numbers[0]
    assert len(compiled) == len(lines) >= 177 + 40
    assert compiled == derived, {k: (compiled.get(k), derived.get(k))
                                 for k in set(compiled) | set(derived)
                                 if compiled.get(k) != derived.get(k)}


vp = C.c_void_p
i32, i64, u64, f64 = C.c_int, C.c_int64, C.c_uint64, C.c_double
# name: (restype, argtypes) as the hand-written table had them before the header was read
FROZEN = {
    'pb_version': (C.c_int, []),
    'pb_timer_read': (C.c_int, [vp, i32, C.c_char_p, i32, C.POINTER(f64)]),
    'pb_lines_stats': (C.c_int, [vp, C.POINTER(i64 * 3)]),
    'pb_voigt_device_bytes': (i64, [vp]),
    'pb_voigt_destroy': (None, [vp]),
    'pb_lbl_kmax_buffer': (C.c_int, [vp, C.POINTER(vp), C.POINTER(i64)]),
    'pb_demc_propose': (C.c_int, [vp, vp, vp, vp, vp, vp, i64, u64, i64, f64, f64, f64, i32, i32,
                                  vp]),
    'pb_cloudy_transit_batch': (C.c_int, [vp, vp, vp, vp, vp, i64, vp, i64, vp, f64, i32, f64, i32,
                                          i32, i32, vp, vp, vp, vp, vp]),
    'pb_lm_update': (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f64, f64, f64, f64, f64,
                               f64, i32, i32, i32, i32, i64, vp]),
    'pb_table_transit_batch': (C.c_int, [vp, vp, vp, vp, vp, vp, vp, f64, i32, i32, f64, i32, i32,
                                         i32, i32, i32, vp, vp]),
}


def _type_class(ctype):
    if ctype is vp or (isinstance(ctype, type) and issubclass(ctype, C._Pointer)):
        return 'pointer'
    return ctype


@pytest.mark.parametrize('name', sorted(FROZEN))
def test_frozen_prototypes(name):
    restype, argtypes = _capi.header().protos[name]
    want_restype, want_argtypes = FROZEN[name]
    assert restype is want_restype
    assert [_type_class(t) for t in argtypes] == [_type_class(t) for t in want_argtypes]
    assert (name in _capi.experiment_names()) == (name == 'pb_table_transit_batch')


GOOD = '''/* a header of the accepted subset */
#ifndef PBHIP_H
#define PBHIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PB_A (-3)   /* a comment
                       over two lines */
#define PB_B 0x10
#define PB_C -2
#define PB_N 3
typedef struct pb_handle pb_handle;
typedef struct pb_x {
    int n, m;
    const double *up_d, *down_d;
    int64_t stride[PB_N];
    uint8_t grid[2][PB_N];
    const int32_t *maps_d[PB_N];
} pb_x;
const char *pb_message(void);
int64_t pb_size(const pb_x *x, pb_handle **out, int64_t stats[3], const double *const *rows_d,
                char *name_out, uint64_t seed);
#ifdef PB_EXPERIMENTS
void pb_trial(double scale);
#endif
#ifdef __cplusplus
}
#endif
#endif
'''


def test_reader_takes_the_stated_subset():
    hdr = _capi.parse_header(GOOD)
    assert hdr.constants == {'PB_A': -3, 'PB_B': 16, 'PB_C': -2, 'PB_N': 3}
    x = hdr.structs['pb_x']
    assert [(n, t) for n, t in x._fields_] == [
        ('n', C.c_int), ('m', C.c_int), ('up_d', vp), ('down_d', vp), ('stride', C.c_int64 * 3),
        ('grid', (C.c_uint8 * 3) * 2), ('maps_d', vp * 3)]
    assert list(hdr.structs) == ['pb_x']
    assert hdr.protos == {'pb_message': (C.c_char_p, []),
                          'pb_size': (C.c_int64, [vp, vp, vp, vp, C.c_char_p, C.c_uint64]),
                          'pb_trial': (None, [C.c_double])}
    assert hdr.experiments == {'pb_trial'}


@pytest.mark.parametrize('before, after, quoted', [
    # a struct field of unknown type
    ('    int n, m;', '    int n, m;\n    float ratio;', 'float ratio;'),
    # a function with a float argument
    ('uint64_t seed);', 'uint64_t seed);\nint pb_scale(double *out_d, float scale);',
     'float scale'),
    # an array bound that names an undefined macro
    ('int64_t stride[PB_N];', 'int64_t stride[PB_UNDEFINED];', 'PB_UNDEFINED'),
    # a declaration outside the grammar: a function-pointer typedef
    ('const char *pb_message(void);',
     'typedef int (*pb_callback)(void *user);\nconst char *pb_message(void);',
     'typedef int (*pb_callback)(void *user);'),
    # (and: a struct by value, an unknown directive, an unknown condition, leftover text)
    ('const pb_x *x,', 'pb_x x,', 'pb_x x'),
    ('#define PB_B 0x10', '#define PB_B 0x10\n#pragma pack(1)', '#pragma pack(1)'),
    ('#ifdef PB_EXPERIMENTS', '#ifdef PB_OTHER', '#ifdef PB_OTHER'),
    ('#define PB_N 3', '#define PB_N 3\n#define PB_M (PB_N + 1)', '#define PB_M (PB_N + 1)'),
    ('} pb_x;', '} pb_x;\nint pb_count', 'int pb_count'),
])
def test_reader_refuses_with_the_text(before, after, quoted):
    """Each text is GOOD with one statement changed; the PbError quotes what it cannot read."""
    assert GOOD.count(before) == 1
    with pytest.raises(_capi.PbError, match=re.escape(quoted)):
        _capi.parse_header(GOOD.replace(before, after))


def test_header_is_read_once(monkeypatch):
    """lib() and the accessors, called repeatedly from a clean start, open the header once."""
    opened = []
    real_open = builtins.open

    def counting_open(file, *args, **kwargs):
        if isinstance(file, (str, os.PathLike)) and os.path.basename(os.fspath(file)) == 'pbhip.h':
            opened.append(file)
        return real_open(file, *args, **kwargs)
    monkeypatch.setattr(_capi, '_header', None)
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setattr(builtins, 'open', counting_open)
    for _ in range(3):
        _capi.lib()
        assert _capi.call('pb_version') >= 100
        assert _capi.constant('PB_ATM_MAX_VMR') == 16
        assert C.sizeof(_capi.struct('pb_radeq_convection')) == 80
        _capi.exported_names(), _capi.experiment_names()
    assert opened == [_capi.HEADER]


def test_missing_header_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_capi, '_header', None)
    monkeypatch.setattr(_capi, 'HEADER', str(tmp_path / 'include' / 'pbhip.h'))
    with pytest.raises(_capi.PbError, match=r'pbhip\.h is missing'):
        _capi.constant('PB_OK')


def test_experiment_entries_follow_the_loaded_library():
    """An entry of the header's experiments section is bound where the library exports it; where
    not, call() says which build carries it."""
    handle = _capi.lib()
    restype, argtypes = _capi.header().protos['pb_table_transit_supported']
    if _capi.experiments():
        assert handle.pb_table_transit_supported.argtypes == argtypes == [C.c_int] * 6
    else:
        with pytest.raises(_capi.PbError) as err:
            _capi.call('pb_table_transit_supported', 1, 1, 2, 0, 2, 2)
        assert str(err.value) == (
            'pb_table_transit_supported is an experiment that libpbhip.so does not carry: build '
            '`make -C pyratbay_amd/csrc EXPERIMENTS=1` and set '
            'PB_LIBPBHIP=pyratbay_amd/libpbhip_exp.so')


def test_status_check_set():
    """call() compares with PB_OK exactly what it compared when the set was written by hand:
    every entry but those below (the entries that do not return int, and the six int-valued
    queries).  pb_last_error, which no table held then, returns a string."""
    unchecked = {
        'pb_version', 'pb_roctx_available',
        'pb_transit_work_doubles', 'pb_two_stream_batch_work_doubles',
        'pb_two_stream_net_work_doubles', 'pb_two_stream_net_parts',
        'pb_weighted_quantiles_work_doubles', 'pb_lm_work_doubles',
        'pb_weighted_quantiles_resident_rows', 'pb_band_contribution_work_doubles',
        'pb_interp_ec_batch_work_doubles', 'pb_interp_ec_batch_cont_work_doubles',
        'pb_table_transit_work_doubles', 'pb_table_transit_supported', 'pb_voigt_destroy',
        'pb_lines_destroy', 'pb_lbl_destroy', 'pb_voigt_device_bytes', 'pb_timer_destroy',
        'pb_lbl_rows_per_step'}
    assert _capi._UNCHECKED == unchecked | {'pb_last_error'}
    protos = _capi.header().protos
    assert {n for n in unchecked if protos[n][0] is C.c_int} == _capi.INT_QUERIES
    assert _capi.PB_OK == 0
