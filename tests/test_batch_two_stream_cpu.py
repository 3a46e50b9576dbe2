"""CPU-only checks of the two-stream walker batch's boundary: libpbhip.so exports
pb_two_stream_batch and pb_two_stream_batch_work_doubles, the scratch size is sane, and every
argument check comes before any HIP call (the pointers handed in are never dereferenced)."""
import ctypes as C

import pytest

NAMES = ('pb_two_stream_batch', 'pb_two_stream_batch_work_doubles')


def test_symbols_exported():
    from pyratbay_amd import _capi
    for name in NAMES:
        assert name in _capi.exported_names() and hasattr(_capi.lib(), name)
    assert _capi.lib().pb_two_stream_batch_work_doubles.restype is C.c_int64


def test_work_doubles():
    """>= 0 everywhere, 0 where nothing is launched or no interval exists, monotone in each
    argument, and beyond 2^31 without wrapping."""
    from pyratbay_amd import _capi
    f = _capi.lib().pb_two_stream_batch_work_doubles
    sizes = (0, 1, 2, 3, 17, 80, 257)
    for L in sizes:
        for W in sizes:
            for nw in sizes:
                v = f(L, W, nw)
                assert v >= 0
                assert f(L + 1, W, nw) >= v and f(L, W + 1, nw) >= v and f(L, W, nw + 1) >= v
                if L <= 1 or W == 0 or nw == 0:
                    assert v == 0
                else:
                    # one transmission per (walker, interval, column)
                    assert v >= nw * (L - 1) * W
    assert f(81, 100000, 512) >= 512 * 80 * 100000 > 2**31


def test_entry_point_checks_arguments_first():
    from pyratbay_amd import _capi
    fake = C.c_void_p(16)          # never dereferenced: the checks come first
    good = [fake, fake, fake, fake, fake, None, None, fake, 12, 100, 4, None]

    def refused(match, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        with pytest.raises(_capi.PbError, match=match):
            _capi.call('pb_two_stream_batch', *args)
        assert match.encode() in _capi.lib().pb_last_error()

    refused('bad shape', a8=0)
    refused('bad shape', a8=-3)
    refused('bad shape', a9=-1)
    refused('bad shape', a10=-1)
    for k in (0, 1, 2, 3, 4):      # flux, ec, intervals, wn, temps
        refused('null pointer', **{f'a{k}': None})
    refused('null work', a7=None)
    refused('layers', a8=1 << 20)
    # one layer has no interval: neither intervals nor work are needed, but the rest is
    refused('null pointer', a8=1, a2=None, a7=None, a0=None)


def test_empty_batches_return_ok():
    """nwalkers == 0 or nwave == 0: status 0 without a launch, whatever the pointers."""
    from pyratbay_amd import _capi
    fake = C.c_void_p(16)
    for L, W, nw in ((12, 0, 4), (12, 100, 0), (1, 0, 0)):
        assert _capi.call('pb_two_stream_batch', fake, fake, fake, fake, fake, None, None, None,
                          L, W, nw, None) == 0
        assert _capi.call('pb_two_stream_batch', None, None, None, None, None, None, None, None,
                          L, W, nw, None) == 0
