"""Device plumbing every module of the front-end shares: the current HIP stream and device
pointers as the C ABI takes them, host array -> device tensor, the process-wide side streams,
stage timers and profiler ranges.  Imports nothing from the package but _capi; importing it
touches neither the GPU nor libpbhip.so."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import call


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_RAW_DEVICE = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
    """The current HIP stream of torch as the `void *stream` of the C ABI.  Every library call
    asks for it; torch.cuda.current_stream() builds a Stream object through several Python layers
    (~8 us, a fifth of the host's submission time of a rank-size spectrum), the raw getters are
    one C call each."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return C.c_void_p(_RAW_STREAM(_RAW_DEVICE()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_SIDE_STREAMS = []


def side_streams(n):
    """The process-wide side streams 0 .. n-1 (created once, shared by every pipeline object).
    HIP maps streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, default 4) in the order
    they are created; two streams on one queue run their kernels strictly one after the other.
    A process that makes fresh streams for every SpectrumPipeline / ShardPipeline soon has two
    "concurrent" contexts on the same queue (seen in a kernel trace: the second of two pipelines
    of one process ran fully serialised).  Re-using the same few streams keeps the mapping the
    one the first pipeline got."""
    while len(_SIDE_STREAMS) < n:
        _SIDE_STREAMS.append(torch.cuda.Stream())
    return _SIDE_STREAMS[:n]


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def dev(a, dtype=torch.float64, device=None):
    """Host array -> contiguous device tensor of the ABI's element type."""
    if isinstance(a, torch.Tensor):
        return a.to(device=device or 'cuda', dtype=dtype).contiguous()
    np_dtype = {torch.float64: np.float64, torch.int32: np.int32,
                torch.int64: np.int64}[dtype]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(device or 'cuda')


def require_gpu():
    if not torch.cuda.is_available():
        raise _capi.PbError('no GPU visible: the HIP path has no CPU fallback')
    _capi.lib()


# --------------------------------------------------------------------------
# Stage timers and profiler ranges
# --------------------------------------------------------------------------
class StageTimer:
    """The reference's `pyrat.timestamps` for the device path (pyrat_obj.py:203-214 with the
    Timer of tools/tools.py:832-843): seconds spent in each named stage since the previous
    mark, measured with HIP events on the launch stream and resolved lazily -- start() and
    mark() only enqueue an event, read() waits for the last one.  Every stage is also a rocTX
    range (rocprofv3 --marker-trace)."""

    def __init__(self, max_stages=8):
        self._h = C.c_void_p()
        call('pb_timer_create', C.byref(self._h), int(max_stages))

    def start(self, first_stage=None):
        call('pb_timer_start', self._h, None if first_stage is None else first_stage.encode(),
             _stream())

    def mark(self, name, next_stage=None):
        call('pb_timer_mark', self._h, name.encode(),
             None if next_stage is None else next_stage.encode(), _stream())

    def read(self):
        """{stage: seconds} of the stages marked since the last start(), in order."""
        n = C.c_int(0)
        call('pb_timer_count', self._h, C.byref(n))
        out = {}
        buf = C.create_string_buffer(64)
        for i in range(n.value):
            sec = C.c_double(0)
            call('pb_timer_read', self._h, i, buf, 64, C.byref(sec))
            key = buf.value.decode()
            out[key] = out.get(key, 0.0) + sec.value
        return out

    def close(self):
        if self._h:
            call('pb_timer_destroy', self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class profiler_range:
    """with profiler_range('all_gather'): ...  -- a rocTX range (no-op without the marker
    library; rocprofv3 --marker-trace shows it beside the kernels)."""

    def __init__(self, name):
        self.name = name.encode()

    def __enter__(self):
        call('pb_range_push', self.name)
        return self

    def __exit__(self, *exc):
        call('pb_range_pop')
        return False
