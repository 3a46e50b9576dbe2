"""The net-flux two-stream batch (k_two_stream_net_batch behind pb_two_stream_net_batch,
csrc/pb_radeq.hip) at the kernel boundary: the bolometric fluxes Qup[L], Qdown[L] -- its parts
summed on the host in the order k_radeq_update adds them -- against np.trapezoid of the oracle
chain's flux_up / flux_down (plane_parallel_optical_depth(inf) -> two_stream), within 1e-12 of
the profile's max(Qup, Qdown); flux_up[0] bit for bit against pb_two_stream_batch; shared against
per-profile f_int / flux_top; the same bits twice.  Every output starts as NaN.

Inputs: test_gpu_two_stream_batch.case (optical depths 1e-3 ... 5 per interval with the special
values of exp1 in the first columns; its docstring).  Shapes L x W x nw: a one-sample grid (the
trapezoid is 0), two samples, a wavefront and one column, one column short of / exactly / one past
a workgroup of 256 (= a part; at 257 the second part has three idle wavefronts), more than one
workgroup with several profiles, L past a wavefront, and L past the 256 threads of the update's
workgroup (300 layers: 26 KB of the kernel's LDS)."""
import functools

import numpy as np
import pytest

import radeq_cases as rc
import test_gpu_two_stream_batch as tsb

pytestmark = pytest.mark.gpu

RTOL = 1e-12
SHAPES = [(2, 1, 1), (2, 2, 1), (3, 65, 1), (9, 255, 1), (9, 256, 1), (9, 257, 1), (70, 600, 3),
          (65, 257, 2), (300, 130, 2)]


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def sources(L, W, nw):
    """Per-profile f_int[nw, W] and flux_top[nw, W]: the shared rows of the case times a factor;
    profile 0 keeps the shared rows."""
    _, _, _, _, f_int, top = tsb.case(L, W, nw)
    scale = 1.0 + 0.5 * np.arange(nw)[:, None]
    return f_int[None] * scale, top[None] / scale


_WANT = {}


def want(orc, L, W, nw, per_profile):
    """(Qup, Qdown [nw, L], flux_up [nw, L, W]) of the oracle chain, once per case."""
    key = (L, W, nw, per_profile)
    if key not in _WANT:
        ecs, intervals, temps, wn, f_int, top = tsb.case(L, W, nw)
        fis, tops = sources(L, W, nw)
        qup, qdown, ups = [], [], []
        for w in range(nw):
            depth = tsb.oracle_depth(orc, ecs[w], intervals[w])
            fi, ft = (fis[w], tops[w]) if per_profile else (f_int, top)
            down, up = orc.two_stream(depth, wn, temps[w], np.ascontiguousarray(fi),
                                      np.ascontiguousarray(ft), 0)
            qup.append(np.trapezoid(up, wn, axis=1))
            qdown.append(np.trapezoid(down, wn, axis=1))
            ups.append(up)
        _WANT[key] = (np.array(qup), np.array(qdown), np.array(ups))
    return _WANT[key]


def run(eng, L, W, nw, per_profile):
    """-> (flux[nw, W], parts[nw, nparts, 2, L]) as device tensors; out, parts and work start as
    NaN, ec is a fresh copy (the call consumes it)."""
    import torch
    from pyratbay_amd import _capi, radeq
    ecs, intervals, temps, wn, f_int, top = tsb.case(L, W, nw)
    fis, tops = sources(L, W, nw)
    fi, ft = (fis, tops) if per_profile else (f_int, top)

    def nan(*shape):
        return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')
    npart = radeq.net_parts(W)
    need = int(_capi.lib().pb_two_stream_net_work_doubles(L, W, nw))
    assert npart == -(-W // 256) and need >= nw * (L - 1) * W
    return radeq.two_stream_net_batch(
        eng.dev(ecs), eng.dev(intervals), eng.dev(wn), eng.dev(radeq.trapezoid_weights(wn)),
        eng.dev(temps), eng.dev(fi), eng.dev(ft), out=nan(nw, W), parts=nan(nw, npart, 2, L),
        work=nan(max(need, 1)))


@pytest.mark.parametrize('per_profile', [False, True])
@pytest.mark.parametrize('L,W,nw', SHAPES)
def test_net_fluxes(eng, orc, L, W, nw, per_profile):
    import torch
    qup_want, qdown_want, ups = want(orc, L, W, nw, per_profile)
    flux, parts = run(eng, L, W, nw, per_profile)
    assert bool(torch.isfinite(parts).all()) and bool(torch.isfinite(flux).all())
    qup, qdown = rc.sum_parts(host(parts))
    for w in range(nw):
        scale = max(qup_want[w].max(), qdown_want[w].max())
        err = max(np.abs(qup[w] - qup_want[w]).max(), np.abs(qdown[w] - qdown_want[w]).max())
        print(f'L={L} W={W} nw={nw} per_profile={per_profile} profile {w}: '
              f'{err / scale if scale > 0 else err:.2e}')
        assert err <= RTOL * scale
        # the ends of the sweeps: the irradiation and flux_down[L-1] + f_int
        tsb.close_by_column(host(flux)[w], ups[w, 0], tsb.RTOL, np.max(np.abs(ups[w]), axis=0))
    if W == 1:
        assert not qup.any() and not qdown.any()       # (a one-sample trapezoid)


@pytest.mark.parametrize('L,W,nw', SHAPES)
def test_spectrum_has_the_bits_of_the_two_stream_batch(eng, L, W, nw):
    """flux_up[0] == pb_two_stream_batch on the same inputs (shared sources: all it takes)."""
    import torch
    ecs, intervals, temps, wn, f_int, top = tsb.case(L, W, nw)
    flux, _ = run(eng, L, W, nw, False)
    ref = eng.two_stream_batch(eng.dev(ecs), eng.dev(intervals), eng.dev(wn), eng.dev(temps),
                               eng.dev(f_int), eng.dev(top))
    assert torch.equal(flux, ref)


def test_shared_against_per_profile_sources(eng):
    """Rows of [nw, W] sources that all equal the shared row give the shared call's bits, and
    profile 0 of the scaled sources (factor 1) equals profile 0 of the shared call."""
    import torch
    from pyratbay_amd import radeq
    L, W, nw = 65, 257, 2
    ecs, intervals, temps, wn, f_int, top = tsb.case(L, W, nw)
    tw = eng.dev(radeq.trapezoid_weights(wn))
    args = [eng.dev(intervals), eng.dev(wn), tw, eng.dev(temps)]
    shared = radeq.two_stream_net_batch(eng.dev(ecs), *args, eng.dev(f_int), eng.dev(top))
    tiled = radeq.two_stream_net_batch(eng.dev(ecs), *args, eng.dev(np.tile(f_int, (nw, 1))),
                                       eng.dev(np.tile(top, (nw, 1))))
    mixed = radeq.two_stream_net_batch(eng.dev(ecs), *args, eng.dev(np.tile(f_int, (nw, 1))),
                                       eng.dev(top))
    none = radeq.two_stream_net_batch(eng.dev(ecs), *args)
    for got in (tiled, mixed):
        assert torch.equal(got[0], shared[0]) and torch.equal(got[1], shared[1])
    scaled = run(eng, L, W, nw, True)
    assert torch.equal(scaled[0][0], shared[0][0]) and torch.equal(scaled[1][0], shared[1][0])
    assert not torch.equal(scaled[1][1], shared[1][1])
    # without sources nothing comes down at the top
    assert not host(none[1])[:, :, 1, 0].any()
    with pytest.raises(ValueError, match='f_int must have shape'):
        radeq.two_stream_net_batch(eng.dev(ecs), *args, eng.dev(np.tile(f_int, (3, 1))))


def test_same_bits_twice_and_guards(eng):
    """A second run, on the first run's leftovers in work, gives the same bits; the rows after
    flux[nw], the parts after the last profile and the tail of work stay untouched."""
    import torch
    from pyratbay_amd import _capi, radeq
    L, W, nw, guard = 70, 600, 3, 64
    ecs, intervals, temps, wn, f_int, top = tsb.case(L, W, nw)
    npart = radeq.net_parts(W)
    need = int(_capi.lib().pb_two_stream_net_work_doubles(L, W, nw))
    work = torch.full((need + guard,), float('nan'), dtype=torch.float64, device='cuda')
    work[need:] = -7.0
    results = []
    for _ in range(2):
        out = torch.full((nw + 1, W), float('nan'), dtype=torch.float64, device='cuda')
        parts = torch.full((nw + 1, npart, 2, L), float('nan'), dtype=torch.float64, device='cuda')
        out[nw], parts[nw] = -7.0, -7.0
        radeq.two_stream_net_batch(eng.dev(ecs), eng.dev(intervals), eng.dev(wn),
                                   eng.dev(radeq.trapezoid_weights(wn)), eng.dev(temps),
                                   eng.dev(f_int), eng.dev(top), out=out[:nw], parts=parts[:nw],
                                   work=work[:need])
        assert bool((out[nw] == -7.0).all()) and bool((parts[nw] == -7.0).all())
        assert bool((work[need:] == -7.0).all()) and bool(torch.isfinite(work[:need]).all())
        results.append((out[:nw].clone(), parts[:nw].clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
