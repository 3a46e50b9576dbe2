"""The four two-stream kernels at the kernel boundary, against 50-digit values of the formulas they
stand for (tests/golden/two_stream_exact.npz, golden/make_golden_two_stream_exact.py): optically
thin layers down to dtau0 = 1e-16, thin above thick, the regime every earlier test drew, and the
special first intervals.  Every element is held to the bound of two_stream_exact_cases.py, which
is derived from rounding counts; the oracle is no reference here -- it keeps the reference's form
of the sweeps' bracket and is wrong by up to 1e13 bounds on these inputs
(test_two_stream_exact_cpu.py).

  pb_two_stream            k_two_stream_trans + k_two_stream: flux_down and flux_up, every layer,
                           rtop = 0 and (17 x 257) rtop = 3
  pb_two_stream_batch      k_two_stream_batch: flux_up[0] per walker from ec and intervals; the
                           bits of the single-spectrum entry on the recomputed depth; ec left as
                           the dtau0 the truth was computed from
  pb_two_stream_net_batch  k_two_stream_net_batch: flux_up[0], and the parts summed in
                           k_radeq_update's order against boundQ, both directions, every layer

On dirty memory: outputs and work buffers start as NaN with a guard behind them, inputs are
compared with their host copies afterwards (ec excepted: the batch entries consume it).  Each test
prints its worst error / bound per class of columns before it asserts (profiles/two_stream.md)."""
import numpy as np
import pytest

import radeq_cases as rc
import two_stream_exact_cases as tc

pytestmark = pytest.mark.gpu

GUARD = -7.0
NGUARD = 64


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def exact(golden):
    return golden('two_stream_exact')


def host(t):
    return t.cpu().numpy()


def dirty(rows, *shape):
    """NaN[rows, *shape] with one more row of GUARD behind it: (the whole tensor, its NaN rows)."""
    import torch
    t = torch.full((rows + 1,) + shape, float('nan'), dtype=torch.float64, device='cuda')
    t[rows] = GUARD
    return t, t[:rows]


def dirty_work(need):
    import torch
    t = torch.full((max(need, 1) + NGUARD,), float('nan'), dtype=torch.float64, device='cuda')
    t[max(need, 1):] = GUARD
    return t, t[:max(need, 1)]


def guard_intact(t, rows):
    return bool((t[rows:] == GUARD).all())


def unchanged(pairs):
    for name, (tensor, array) in pairs.items():
        assert np.array_equal(host(tensor), array), f'{name} was written to'


class Ledger:
    """Holds every element to its bound, printing each figure first; the assertion comes in
    close(), after all of a test's figures are out (profiles/two_stream.md lists them)."""

    def __init__(self):
        self.failed = []

    def held(self, what, got, want, bound):
        """The worst error / bound per class of columns.  got, want: [W] or [L, W]; bound: [W]."""
        over = tc.worst_over_bound(np.atleast_2d(got), np.atleast_2d(want), bound)
        cls = tc.column_class(len(bound))
        by_class = {name: float(over[cls == c].max()) for c, name in enumerate(tc.CLASSES)}
        print(f'{what}: worst error / bound ' +
              ', '.join(f'{name} {v:.3g}' for name, v in by_class.items()))
        if not np.all(over <= 1.0):
            self.failed.append((what, by_class, int(np.argmax(over))))

    def held_sums(self, what, got, want, bound_q):
        """Bolometric sums [L] against boundQ [L]."""
        with np.errstate(invalid='ignore'):
            over = np.where(np.isfinite(got), np.abs(got - want) / bound_q, np.inf)
        print(f'{what}: worst sum error / boundQ {over.max():.3g}')
        if not np.all(over <= 1.0):
            self.failed.append((what, float(over.max()), int(np.argmax(over))))

    def close(self):
        assert not self.failed, self.failed


def device_inputs(eng, exact, L, W):
    """The shape's inputs as device tensors with the host arrays they came from."""
    wn, f_int, top, tw = tc.shared_inputs(exact, L, W)
    walkers = [tc.walker_inputs(exact, L, W, w) for w in range(tc.NWALKERS)]
    arrays = dict(wn=wn, f_int=f_int, flux_top=top, tw=tw,
                  ec=np.array([w[0] for w in walkers]),
                  intervals=np.array([w[1] for w in walkers]),
                  temp=np.array([w[2] for w in walkers]))
    return {k: (eng.dev(v), v) for k, v in arrays.items()}


@pytest.mark.parametrize('L,W,walker,rtop', tc.cases())
def test_single_spectrum_entry(eng, exact, L, W, walker, rtop):
    """pb_two_stream on the recomputed depth: both directions, every layer."""
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    d = device_inputs(eng, exact, L, W)
    ec, h, temp = tc.walker_inputs(exact, L, W, walker)
    depth, _ = tc.depth_of(ec, h)
    down_want, up_want, _, _ = tc.truth(exact, L, W, walker, rtop)
    bnd = tc.bound(d['wn'][1], temp, down_want, up_want)
    ins = dict(depth=(eng.dev(depth), depth), temp=(eng.dev(temp), temp), wn=d['wn'],
               f_int=d['f_int'], flux_top=d['flux_top'])
    down_all, down = dirty(L, W)
    up_all, up = dirty(L, W)
    _capi.call('pb_two_stream', _ptr(down), _ptr(up), _ptr(ins['depth'][0]), _ptr(ins['wn'][0]),
               _ptr(ins['temp'][0]), _ptr(ins['f_int'][0]), _ptr(ins['flux_top'][0]), rtop, L, W,
               _stream())
    assert guard_intact(down_all, L) and guard_intact(up_all, L)
    unchanged(ins)
    tag = f'pb_two_stream L={L} W={W} walker {walker} rtop={rtop}'
    ledger = Ledger()
    ledger.held(tag + ' down', host(down), down_want, bnd)
    ledger.held(tag + ' up', host(up), up_want, bnd)
    # the front end's call is the same call
    down2, up2 = eng.two_stream(ins['depth'][0], ins['wn'][0], ins['temp'][0], ins['f_int'][0],
                                ins['flux_top'][0], rtop)
    assert torch.equal(down2, down) and torch.equal(up2, up)
    ledger.close()


@pytest.mark.parametrize('L,W', tc.SHAPES)
def test_batch_entry(eng, exact, L, W):
    """pb_two_stream_batch: flux_up[0] of both walkers from ec and intervals."""
    import torch
    from pyratbay_amd import _capi
    nw = tc.NWALKERS
    d = device_inputs(eng, exact, L, W)
    need = int(_capi.lib().pb_two_stream_batch_work_doubles(L, W, nw))
    assert need >= nw * (L - 1) * W
    out_all, out = dirty(nw, W)
    work_all, work = dirty_work(need)
    ec = d['ec'][0].clone()
    got = eng.two_stream_batch(ec, d['intervals'][0], d['wn'][0], d['temp'][0], d['f_int'][0],
                               d['flux_top'][0], out=out, work=work[:need])
    assert got.data_ptr() == out.data_ptr()
    assert guard_intact(out_all, nw) and guard_intact(work_all, max(need, 1))
    unchanged({k: d[k] for k in ('intervals', 'wn', 'temp', 'f_int', 'flux_top')})
    ledger = Ledger()
    for w in range(nw):
        ec_w, h, temp = tc.walker_inputs(exact, L, W, w)
        depth, dtau0 = tc.depth_of(ec_w, h)
        down_want, up_want, _, _ = tc.truth(exact, L, W, w)
        bnd = tc.bound(d['wn'][1], temp, down_want, up_want)
        # what the kernel leaves in ec is the dtau0 the truth was computed from
        assert np.array_equal(host(ec[w, :L - 1]), dtau0)
        ledger.held(f'pb_two_stream_batch L={L} W={W} walker {w} flux_up[0]', host(out[w]),
                    up_want[0], bnd)
        one = eng.two_stream(eng.dev(depth), d['wn'][0], d['temp'][0][w], d['f_int'][0],
                             d['flux_top'][0], 0)[1][0]
        assert torch.equal(out[w], one), f'walker {w}: not the bits of the single-spectrum entry'
    ledger.close()


@pytest.mark.parametrize('L,W', tc.SHAPES)
def test_net_batch_entry(eng, exact, L, W):
    """pb_two_stream_net_batch: flux_up[0], and Qup / Qdown of every layer from the parts."""
    import torch
    from pyratbay_amd import _capi, radeq
    nw = tc.NWALKERS
    d = device_inputs(eng, exact, L, W)
    assert np.array_equal(d['tw'][1], radeq.trapezoid_weights(d['wn'][1]))
    npart = radeq.net_parts(W)
    assert npart == -(-W // tc.PART)
    if (L, W) == tc.RTOP_SHAPE:
        assert npart == 2 and W - tc.PART == 1       # (one live column in the second part)
    need = int(_capi.lib().pb_two_stream_net_work_doubles(L, W, nw))
    assert need >= nw * (L - 1) * W
    out_all, out = dirty(nw, W)
    parts_all, parts = dirty(nw, npart, 2, L)
    work_all, work = dirty_work(need)
    ec = d['ec'][0].clone()
    radeq.two_stream_net_batch(ec, d['intervals'][0], d['wn'][0], d['tw'][0], d['temp'][0],
                               d['f_int'][0], d['flux_top'][0], out=out, parts=parts,
                               work=work[:max(need, 1)])
    assert guard_intact(out_all, nw) and guard_intact(parts_all, nw)
    assert guard_intact(work_all, max(need, 1))
    unchanged({k: d[k] for k in ('intervals', 'wn', 'tw', 'temp', 'f_int', 'flux_top')})
    assert bool(torch.isfinite(parts).all())
    q_up, q_down = rc.sum_parts(host(parts))
    tw = d['tw'][1]
    ledger = Ledger()
    for w in range(nw):
        _, _, temp = tc.walker_inputs(exact, L, W, w)
        down_want, up_want, q_down_want, q_up_want = tc.truth(exact, L, W, w)
        bnd = tc.bound(d['wn'][1], temp, down_want, up_want)
        tag = f'pb_two_stream_net_batch L={L} W={W} walker {w}'
        ledger.held(tag + ' flux_up[0]', host(out[w]), up_want[0], bnd)
        ledger.held_sums(tag + ' Qup', q_up[w], q_up_want, tc.bound_q(tw, bnd, up_want))
        ledger.held_sums(tag + ' Qdown', q_down[w], q_down_want, tc.bound_q(tw, bnd, down_want))
    ref = eng.two_stream_batch(d['ec'][0].clone(), d['intervals'][0], d['wn'][0], d['temp'][0],
                               d['f_int'][0], d['flux_top'][0])
    assert torch.equal(out, ref)
    ledger.close()
