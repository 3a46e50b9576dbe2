"""ctypes binding of libpbhip.so (include/pbhip.h).

There is no CPU fallback: if the shared library is missing or a call fails, an
exception is raised.  torch is used only as plumbing for device memory and streams.
"""
import collections
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PB_LIBPBHIP=<path>: another build of the library -- libpbhip_exp.so (`make EXPERIMENTS=1`: the
# product + the measured dead ends) or one of the debug builds of tools/debug/
LIBPATH = os.environ.get('PB_LIBPBHIP') or os.path.join(_HERE, 'libpbhip.so')


class PbError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------
# include/pbhip.h is the one statement of the boundary: constants, structs and prototypes are read
# from it (its opening comment names the subset of C this reader takes).  Whatever the reader
# does not recognise raises -- nothing is skipped, or the reader would be a copy that can drift.
# ---------------------------------------------------------------------------------------------
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'pbhip.h')

_SCALARS = {'int': C.c_int, 'int16_t': C.c_int16, 'int32_t': C.c_int32, 'int64_t': C.c_int64,
            'uint64_t': C.c_uint64, 'uint8_t': C.c_uint8, 'double': C.c_double}
_RETURNS = {'int': C.c_int, 'int64_t': C.c_int64, 'void': None, 'const char *': C.c_char_p}
# The entries whose int is a value.  Every other entry that returns int returns a status, which
# call() checks against PB_OK.
INT_QUERIES = frozenset((
    'pb_version', 'pb_roctx_available', 'pb_two_stream_net_parts',
    'pb_weighted_quantiles_resident_rows', 'pb_lbl_rows_per_step', 'pb_table_transit_supported'))

_STATEMENT = re.compile(r"""\s*(?:
      typedef\s+struct\s+(?P<tag>\w+)\s*(?:\{(?P<body>[^{}]*)\})?\s*(?P<alias>\w+)\s*;
    | (?P<ret>[\w\s*]+?)\s*\b(?P<fn>\w+)\s*\((?P<args>[^(){};]*)\)\s*;
    )""", re.X)
_FIELD = re.compile(r'(?:const\s+)?(\w+)\b\s*(.+)', re.S)
_DECLARATOR = re.compile(r'\s*(\**)\s*(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)')
_PARAM = re.compile(
    r'(?:const\s+)?(\w+)\b\s*((?:\*\s*(?:const\b\s*)?)*)\b\w+\s*((?:\[\s*\w*\s*\])*)')

Header = collections.namedtuple('Header', 'constants structs protos experiments')


def _quote(text):
    return ' '.join(text.split())


def _integer(text, what):
    inner = text[1:-1] if text.startswith('(') and text.endswith(')') else text
    try:
        return int(inner.strip(), 0)
    except ValueError:
        raise PbError(f'pbhip.h: {what} is not an integer') from None


def _fields(tag, body, constants, pointees):
    """The _fields_ of one struct body."""
    fields = []
    for statement in filter(None, map(str.strip, body.split(';'))):
        m = _FIELD.fullmatch(statement)
        decls = [_DECLARATOR.fullmatch(d) for d in m.group(2).split(',')] if m else [None]
        if None in decls:
            raise PbError(f'pbhip.h: struct {tag}: cannot read `{_quote(statement)};`')
        base = m.group(1)
        for stars, name, dims in (d.groups() for d in decls):
            if base not in (pointees if stars else _SCALARS):
                raise PbError(f'pbhip.h: struct {tag}: unknown type `{base}` in '
                              f'`{_quote(statement)};`')
            ctype = C.c_void_p if stars else _SCALARS[base]
            for bound in reversed(re.findall(r'\w+', dims)):
                n = int(bound) if bound.isdigit() else constants.get(bound)
                if n is None or n <= 0:
                    raise PbError(f'pbhip.h: struct {tag}: array bound `{bound}` of '
                                  f'`{_quote(statement)};` is not a positive integer or a '
                                  'constant defined in the header')
                ctype = ctype * n
            fields.append((name, ctype))
    return fields


def _argtype(fn, param, pointees):
    m = _PARAM.fullmatch(param.strip())
    if not m:
        raise PbError(f'pbhip.h: {fn}: cannot read the parameter `{_quote(param)}`')
    base, stars, dims = m.groups()
    pointer = bool(stars or dims)
    if base not in (pointees if pointer else _SCALARS):
        raise PbError(f'pbhip.h: {fn}: unknown type in the parameter `{_quote(param)}`')
    if not pointer:
        return _SCALARS[base]
    return C.c_char_p if base == 'char' and stars.count('*') == 1 and not dims else C.c_void_p


def parse_header(text):
    """Header(constants {name: int}, structs {name: Structure subclass}, protos {name: (restype,
    argtypes)}, experiments: the names declared under #ifdef PB_EXPERIMENTS) of the text of
    pbhip.h.  PbError, quoting the text, for anything outside the subset the header states."""
    constants, structs, protos, experiments = {}, {}, {}, set()
    code = {None: [], 'PB_EXPERIMENTS': [], '__cplusplus': []}
    conditions = []
    for line in re.sub(r'/\*.*?\*/', ' ', text, flags=re.S).split('\n'):
        m = re.match(r'\s*#\s*(\w+)\s*(.*?)\s*$', line)
        if not m:
            code[next((c for c in ('__cplusplus', 'PB_EXPERIMENTS') if c in conditions),
                      None)].append(line)
            continue
        directive, rest = m.groups()
        define = re.fullmatch(r'(\w+)(?:\s+(.+))?', rest) if directive == 'define' else None
        if directive in ('ifdef', 'ifndef') and \
                rest in ('PBHIP_H', '__cplusplus', 'PB_EXPERIMENTS'):
            conditions.append(rest)
        elif directive == 'endif' and conditions:
            conditions.pop()
        elif define:
            if define.group(2) is not None:     # (without a value: the include guard)
                constants[define.group(1)] = _integer(define.group(2), f'`{_quote(line)}`')
        elif (directive, rest) != ('include', '<stdint.h>'):
            raise PbError(f'pbhip.h: cannot read the preprocessor line `{_quote(line)}`')
    if conditions:
        raise PbError(f'pbhip.h: `#ifdef {conditions[-1]}` is not closed')
    for piece in filter(None, map(_quote, code['__cplusplus'])):
        if piece not in ('extern "C" {', '}'):
            raise PbError(f'pbhip.h: cannot read `{piece}` under #ifdef __cplusplus')
    pointees = set(_SCALARS) | {'void', 'char'}     # what a pointer may point to
    for section in (None, 'PB_EXPERIMENTS'):
        source, pos = '\n'.join(code[section]), 0
        while source[pos:].strip():
            m = _STATEMENT.match(source, pos)
            if not m:
                raise PbError('pbhip.h: cannot read the declaration '
                              f'`{_quote(source[pos:].split(";")[0])};`')
            pos = m.end()
            tag, fn = m.group('tag'), m.group('fn')
            if tag:
                if tag != m.group('alias') or tag in pointees:
                    raise PbError(f'pbhip.h: cannot read the declaration `{_quote(m.group())}`')
                pointees.add(tag)
                if m.group('body') is not None:
                    structs[tag] = type(tag, (C.Structure,), {
                        '__doc__': f'{tag} of include/pbhip.h.',
                        '_fields_': _fields(tag, m.group('body'), constants, pointees)})
                continue
            ret = ' '.join(m.group('ret').replace('*', ' * ').split())
            if ret not in _RETURNS or fn in protos:
                raise PbError(f'pbhip.h: cannot read the declaration `{_quote(m.group())}`')
            args = m.group('args').strip()
            protos[fn] = (_RETURNS[ret], [] if args == 'void' else
                          [_argtype(fn, p, pointees) for p in args.split(',')])
            if section:
                experiments.add(fn)
    return Header(constants, structs, protos, experiments)


_header = None


def header():
    """include/pbhip.h, read once per process."""
    global _header
    if _header is None:
        if not os.path.exists(HEADER):
            raise PbError(f'{HEADER} is missing: the binding reads its constants, structs and '
                          'prototypes from it')
        with open(HEADER) as f:
            parsed = parse_header(f.read())
        stray = sorted(n for n in INT_QUERIES if parsed.protos.get(n, (None,))[0] is not C.c_int)
        if stray:
            raise PbError(f'pbhip.h: {stray} of _capi.INT_QUERIES are not declared as int')
        _header = parsed
    return _header


def constant(name):
    """The value of `#define <name>` of include/pbhip.h."""
    try:
        return header().constants[name]
    except KeyError:
        raise PbError(f'pbhip.h defines no constant {name}') from None


def struct(name):
    """The ctypes.Structure of `typedef struct <name> { ... } <name>;` of include/pbhip.h."""
    try:
        return header().structs[name]
    except KeyError:
        raise PbError(f'pbhip.h defines no struct {name}') from None


PB_OK = constant('PB_OK')
# what call() does not compare with PB_OK: every entry that does not return int, and INT_QUERIES
_UNCHECKED = INT_QUERIES | {n for n, (restype, _) in header().protos.items()
                            if restype is not C.c_int}
_lib = None


def exported_names():
    return sorted(set(header().protos) - header().experiments)


def experiment_names():
    """The entries of libpbhip_exp.so only (include/pbhip.h, "Experiments"): bound when the loaded
    library has them."""
    return sorted(header().experiments)


def experiments():
    """True when the loaded library is the experiments build (libpbhip_exp.so)."""
    return hasattr(lib(), 'pb_table_transit_batch')


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  torch bundles its own libamdhip64 (SONAME
    libamdhip64.so.7, file name libamdhip64.so); libpbhip.so needs the same SONAME.  If
    libpbhip were loaded first it would pull /opt/rocm's copy and torch would later add
    its own: two runtimes, and device pointers / streams handed across would break.
    Loading torch's copy first makes the dynamic loader reuse it for libpbhip."""
    import torch
    cand = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load libpbhip.so or fail loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise PbError(
                f'{LIBPATH} is missing: build it with `make -C pyratbay_amd/csrc` '
                '(or __graft_entry__.build()); there is no CPU fallback')
        _preload_torch_hip_runtime()
        handle = C.CDLL(LIBPATH)
        for name, (restype, argtypes) in header().protos.items():
            fn = getattr(handle, name, None) if name in header().experiments else \
                getattr(handle, name)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
        global _owner_pid
        _owner_pid = os.getpid()
    return _lib


_owner_pid = None


def call(name, *args):
    # The reference parallelises with fork (pyrat/line_by_line.py:232-246, ncpu > 1).  A
    # forked child of a process that has initialised HIP cannot use the GPU (and on this
    # platform must not try): fail loudly instead of hanging or faulting.
    if _owner_pid is not None and os.getpid() != _owner_pid:
        raise PbError(f'{name}: called in a forked child (pid {os.getpid()}) of the process '
                      f'that initialised the GPU (pid {_owner_pid}); the HIP path needs '
                      'ncpu = 1 -- it batches all layers in one call instead of forking')
    fn = getattr(lib(), name, None)
    if fn is None:
        raise PbError(f'{name} is an experiment that libpbhip.so does not carry: build '
                      '`make -C pyratbay_amd/csrc EXPERIMENTS=1` and set '
                      'PB_LIBPBHIP=pyratbay_amd/libpbhip_exp.so')
    rc = fn(*args)
    if name not in _UNCHECKED and rc != PB_OK:
        raise PbError(f'{name} failed ({rc}): {lib().pb_last_error().decode()}')
    return rc


def hptr(a):
    """Host pointer of a C-contiguous NumPy array (or None)."""
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def f64h(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32h(a):
    return np.ascontiguousarray(a, dtype=np.int32)
