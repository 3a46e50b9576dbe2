"""Every form of the batched interpolation (csrc/pb_interp.hip: plan_interp + launch_interp) at
small shapes: chunks of more than one walker (the bracket walk across a chunk), two pair slots per
thread by the rule and forced, unaligned bases, every species instantiation.  Each walker against
the one-walker kernel (pb_interp_ec_set: bit for bit) and the oracle's interp_ec (RTOL), on an
output buffer pre-filled with a sentinel.  The PB_INTERP_* switches are read at every call, so a
test sets them for its own calls; which form a call takes is asked of pb_interp_ec_batch_plan."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-12
SENTINEL = -7.0
VARS = ('PB_INTERP_CHUNK', 'PB_INTERP_PAIRS', 'PB_INTERP_NP', 'PB_INTERP_FULL')


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


def host(t):
    return t.cpu().numpy()


def plan(nmol, L, W, nw, aligned=True):
    from pyratbay_amd import _capi
    out = (C.c_int32 * 6)()
    _capi.call('pb_interp_ec_batch_plan', out, nmol, L, W, nw, int(aligned), 0, 0)
    return dict(zip(('chunk', 'pairs', 'slots', 'kS', 'kFull', 'gx'), out))


def make_case(seed, nmol, ntemp, L, W, nw):
    """Table 10**U(-30, -20) on linspace(300, 3000, ntemp); walker 0 on nodes, 1 at 300 K, 2 at
    3000 K, 3 in one bracket; from walker 4 on, in every run of four consecutive walkers (a chunk
    of the launches below, or part of one) the second shares the first's bracket at every layer,
    and in every other run the walkers sit in the brackets 0, 0, 2 and 4 (ntemp >= 6): the
    brackets 1 and 3 lie between the run's lowest and highest and are used by none of them."""
    rng = np.random.default_rng(seed)
    ttable = np.linspace(300.0, 3000.0, ntemp)
    etable = 10.0**rng.uniform(-30, -20, (nmol, ntemp, L, W))
    temps = rng.uniform(300.0, 3000.0, (nw, L))
    temps[0] = ttable[rng.integers(0, ntemp, L)]
    if nw > 3:
        temps[1] = 300.0
        temps[2] = 3000.0
        temps[3] = np.linspace(640, 660, L)

    def inside(b):
        return ttable[b] + (ttable[b + 1] - ttable[b]) * rng.uniform(0.05, 0.95, L)
    for w0 in range(4, nw - 3, 4):
        if ntemp >= 6 and (w0 // 4) % 2 == 0:
            for k, b in enumerate((0, 0, 2, 4)):
                temps[w0 + k] = inside(b)
        else:
            b = np.clip(np.searchsorted(ttable, temps[w0], 'right') - 1, 0, ntemp - 2)
            temps[w0 + 1] = inside(b)
    dens = 10.0**rng.uniform(8, 18, (nw, L, nmol))
    return dict(nmol=nmol, ntemp=ntemp, L=L, W=W, nw=nw, ttable=ttable, etable=etable,
                temps=temps, dens=dens)


def device(eng, c):
    return dict(et=eng.dev(c['etable']), tt=eng.dev(c['ttable']), td=eng.dev(c['temps']),
                dd=eng.dev(c['dens']))


def batch(eng, c, d, out=None, et=None):
    import torch
    if out is None:
        out = torch.full((c['nw'], c['L'], c['W']), SENTINEL, dtype=torch.float64, device='cuda')
    eng.interp_ec_batch(d['et'] if et is None else et, d['tt'], d['td'], d['dd'], out=out)
    return host(out)


def singles(eng, c, d):
    """The one-walker kernel, walker by walker."""
    import torch
    want = np.empty((c['nw'], c['L'], c['W']))
    for w in range(c['nw']):
        one = torch.full((c['L'], c['W']), 3.3, dtype=torch.float64, device='cuda')
        eng.interp_ec(one, d['et'], d['tt'], d['td'][w], d['dd'][w], 0, c['L'], assign=True)
        want[w] = host(one)
    return want


def check(orc, c, got, want):
    assert not np.any(got == SENTINEL)
    for w in range(c['nw']):
        assert np.array_equal(got[w], want[w]), w           # same arithmetic, bit for bit
    nw = c['nw']
    for w in sorted(set(range(min(nw, 4))) | {w for w in (4, 5, 10, nw - 1) if 0 <= w < nw}):
        ref = np.zeros((c['L'], c['W']))
        orc.interp_ec(ref, c['etable'], c['ttable'], c['temps'][w], c['dens'][w], 0, c['L'])
        np.testing.assert_allclose(got[w], ref, rtol=RTOL)


@pytest.mark.parametrize('L,chunk', [(32, 4), (31, 2)])
def test_chunks_above_one(eng, orc, L, chunk):
    """64 walkers x 770 samples: 32 layers run in chunks of 4 walkers, 31 in chunks of 2 -- the
    bracket walk across the walkers of a chunk, with shared, distinct and skipped brackets."""
    c = make_case(11, 4, 7, L, 770, 64)
    p = plan(4, L, 770, 64)
    assert (p['chunk'], p['pairs'], p['slots']) == (chunk, 1, 1)
    tlo = np.clip(np.searchsorted(c['ttable'], c['temps'], 'right') - 1, 0, 5)
    assert np.all(tlo[4] == tlo[5]) and np.all(tlo[12] == tlo[13])
    assert np.all(tlo[8:12] == np.array([0, 0, 2, 4])[:, None])
    d = device(eng, c)
    check(orc, c, batch(eng, c, d), singles(eng, c, d))


@pytest.mark.parametrize('W,slots,gx', [(31742, 2, 32), (31738, 1, 62)])
def test_two_slots_by_the_rule(eng, orc, W, slots, gx):
    """One species, 2 walkers x 128 layers: at 31 742 samples the launch still has 4096 workgroups
    of two pair slots per thread, at 31 738 it has not."""
    c = make_case(12, 1, 3, 128, W, 2)
    p = plan(1, 128, W, 2)
    assert (p['chunk'], p['pairs'], p['slots'], p['gx']) == (64, 1, slots, gx)
    d = device(eng, c)
    check(orc, c, batch(eng, c, d), singles(eng, c, d))


@pytest.mark.parametrize('L,W', [(9, 1500), (8, 1501), (8, 5), (10, 258), (8, 1023), (8, 1025),
                                 (8, 1026)])
def test_two_slots_forced(eng, orc, monkeypatch, L, W):
    """PB_INTERP_NP=2 at small shapes: rows that start at even and at odd elements, one pair, a
    pair in the second slot, and 1023 / 1025 / 1026 samples around the 512 slots of a workgroup of
    this form.  The same bits as one slot per thread and as one sample per thread."""
    c = make_case(13 + W, 4, 7, L, W, 5)
    d = device(eng, c)
    monkeypatch.setenv('PB_INTERP_NP', '2')
    p = plan(4, L, W, 5)
    assert (p['pairs'], p['slots']) == (1, 2)
    assert p['gx'] == -(-(W // 2 + 2) // 512)
    two = batch(eng, c, d)
    monkeypatch.setenv('PB_INTERP_NP', '1')
    assert plan(4, L, W, 5)['slots'] == 1
    one = batch(eng, c, d)
    monkeypatch.delenv('PB_INTERP_NP')
    monkeypatch.setenv('PB_INTERP_PAIRS', '0')
    assert plan(4, L, W, 5)['pairs'] == 0
    single = batch(eng, c, d)
    check(orc, c, two, singles(eng, c, d))
    assert np.array_equal(one, two) and np.array_equal(single, two)


def test_unaligned_bases(eng, orc):
    """ec, then the table, one double into a larger buffer (8 mod 16): the one-sample kernel runs,
    with the bits of the aligned call, and the doubles around the view are left alone."""
    import torch
    L, W, nw = 8, 1500, 5
    c = make_case(14, 4, 7, L, W, nw)
    d = device(eng, c)
    assert plan(4, L, W, nw)['pairs'] == 1 and plan(4, L, W, nw, aligned=False)['pairs'] == 0
    aligned = batch(eng, c, d)
    check(orc, c, aligned, singles(eng, c, d))
    n = nw * L * W
    buf = torch.full((n + 2,), SENTINEL, dtype=torch.float64, device='cuda')
    out = buf[1:n + 1].view(nw, L, W)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 8
    got = batch(eng, c, d, out=out)
    assert np.array_equal(got, aligned)
    assert float(buf[0]) == SENTINEL and float(buf[-1]) == SENTINEL
    ne = c['etable'].size
    ebuf = torch.full((ne + 2,), SENTINEL, dtype=torch.float64, device='cuda')
    et = ebuf[1:ne + 1].view(c['etable'].shape)
    et.copy_(d['et'])
    assert ebuf.data_ptr() % 16 == 0 and et.data_ptr() % 16 == 8
    assert np.array_equal(batch(eng, c, d, et=et), aligned)
    assert float(ebuf[0]) == SENTINEL and float(ebuf[-1]) == SENTINEL


@pytest.mark.parametrize('form', ['one_sample', 'default', 'two_slots'])
@pytest.mark.parametrize('nmol', [1, 3, 4, 5, 8])
def test_species(eng, orc, monkeypatch, nmol, form):
    """Every species instantiation (4 / 8 in registers, with and without the per-species
    predicate) in every form; four species with PB_INTERP_FULL=0 give the bits they give
    without it."""
    L, W, nw = 8, 1500, 5
    c = make_case(15 + nmol, nmol, 7, L, W, nw)
    d = device(eng, c)
    if form == 'one_sample':
        monkeypatch.setenv('PB_INTERP_PAIRS', '0')
    elif form == 'two_slots':
        monkeypatch.setenv('PB_INTERP_NP', '2')
    p = plan(nmol, L, W, nw)
    assert (p['pairs'], p['slots']) == {'one_sample': (0, 1), 'default': (1, 1),
                                        'two_slots': (1, 2)}[form]
    assert (p['kS'], p['kFull']) == {1: (4, 0), 3: (4, 0), 4: (4, 1), 5: (8, 0), 8: (8, 1)}[nmol]
    got = batch(eng, c, d)
    check(orc, c, got, singles(eng, c, d))
    if nmol == 4:
        monkeypatch.setenv('PB_INTERP_FULL', '0')
        assert plan(nmol, L, W, nw)['kFull'] == 0
        assert np.array_equal(batch(eng, c, d), got)
