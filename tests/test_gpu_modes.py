"""The mode decomposition on the device (csrc/pb_modes.hip, NestedSampler.modes) against its NumPy
statements (pyratbay_amd/modes.py), at the C ABI into dirty outputs with a guard behind them:

  * pb_modes_sqdist, pb_modes_link, pb_modes_assign and pb_modes_rows against sqdist_host,
    link_host, assign_host and rows_host with np.array_equal, on every hand-made case of
    modes_cases;
  * pb_modes_evidence against evidence_host on nested_cases' finish inputs split at random into
    modes: the special values exactly, the others to 1e-12 -- the device's exp and log are not the
    host's to the last bit, the one thing here no order of operations settles (pb_nested_finish is
    tested the same way; measured: 59 of 60 values have the host's bits, one fraction is off by
    one unit in its last place, 5.4e-20);
  * every refusal;
  * NestedSampler.modes on the two-mode target, bit for bit against modes_host applied to the
    read-back state of the same run (the local evidences too), and within the committed bounds of
    the closed form;
  * unique(mode=) and Retrieval.summary(mode=) on test_gpu_retrieval's small emission model."""
import types

import numpy as np
import pytest

import modes_cases as mc
import sampler_cases as sc
from test_gpu_sampler import no_read_back

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def nan_tensor(shape):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')


def int_tensor(shape, kind='int32', value=-77):
    import torch
    return torch.full(shape, value, dtype=getattr(torch, kind), device='cuda')


def dev_i32(eng, a):
    import torch
    return eng.dev(np.asarray(a), torch.int32)


# -------------------------------------------------------------------------------------------------
# the kernels at the C ABI
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nfree', [1, 3, 16, 17, 128])
def test_sqdist_against_the_host_statement(eng, nfree):
    import torch
    from pyratbay_amd import _capi, modes
    from pyratbay_amd._device import _ptr, _stream
    rng = np.random.default_rng(nfree)
    for na, nb in ((1, 1), (63, 31), (64, 32), (65, 33), (300, 65),
                   (257, 4096 if nfree == 3 else 97)):
        A, B = rng.uniform(0, 1, (na, nfree)), rng.uniform(0, 1, (nb, nfree))
        d2 = nan_tensor((na + 1, nb))
        A_d, B_d = eng.dev(A), eng.dev(B)
        _capi.call('pb_modes_sqdist', _ptr(d2), _ptr(A_d), _ptr(B_d), na, nb, nfree, _stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(d2[na]).all())
        assert np.array_equal(bits(host(d2[:na])), bits(modes.sqdist_host(A, B))), (na, nb)


def run_link(eng, R, knn=10, link=1.0, min_mode=None, max_modes=16):
    import torch
    from pyratbay_amd import _capi, modes
    from pyratbay_amd._device import _ptr, _stream
    n, nfree = R.shape
    min_mode = modes.default_min_mode(nfree) if min_mode is None else min_mode
    nwords = (n + 31) // 32
    labels, nmodes = int_tensor((n + 1,)), int_tensor((2,))
    ell2, dk = nan_tensor((2,)), nan_tensor((n + 1,))
    work = int_tensor((n * nwords + 1,), value=0x5a5a5a5a)
    R_d = eng.dev(R)
    _capi.call('pb_modes_link', _ptr(labels), _ptr(nmodes), _ptr(ell2), _ptr(dk), _ptr(work),
               _ptr(R_d), n, nfree, knn, link, min_mode, max_modes, _stream())
    torch.cuda.synchronize()
    assert int(labels[n]) == -77 and int(nmodes[1]) == -77 and int(work[n * nwords]) == 0x5a5a5a5a
    assert bool(torch.isnan(ell2[1])) and bool(torch.isnan(dk[n]))
    assert np.array_equal(bits(host(R_d)), bits(R))
    return host(labels[:n]), int(nmodes[0]), float(ell2[0])


LINK_CASES = mc.link_cases()


@pytest.mark.parametrize('kind', mc.KINDS)
def test_link_against_the_host_statement(eng, kind):
    from pyratbay_amd import modes
    seen = set()
    for name, R, kw, expect in LINK_CASES:
        if not name.startswith(kind + '-'):
            continue
        want, want_nmodes, want_ell2 = modes.link_host(R, **kw)
        labels, nmodes, ell2 = run_link(eng, R, **kw)
        assert np.array_equal(labels, want), name
        assert nmodes == want_nmodes and bits(ell2) == bits(want_ell2), name
        if expect is not None:
            assert nmodes == expect, name
        seen.add(nmodes)
    assert seen


def run_assign(eng, P, R, labels):
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    N, nfree = P.shape
    mode = int_tensor((N + 1,))
    P_d, R_d, labels_d = eng.dev(P), eng.dev(R), dev_i32(eng, labels)
    _capi.call('pb_modes_assign', _ptr(mode), _ptr(P_d), _ptr(R_d), _ptr(labels_d), N, len(R),
               nfree, _stream())
    torch.cuda.synchronize()
    assert int(mode[N]) == -77
    return host(mode[:N])


@pytest.mark.parametrize('nfree', mc.LINK_NFREES)
def test_assign_against_the_host_statement(eng, nfree):
    from pyratbay_amd import modes
    for variant in ('modes', 'loose'):
        for N in mc.ASSIGN_NS:
            P, R, labels = mc.assign_case(N, nfree, variant)
            want = modes.assign_host(P, R, labels)
            assert np.array_equal(run_assign(eng, P, R, labels), want), (variant, N)
            if N == 1000:
                assert set(want) == ({0} if variant == 'loose' else {0, 1})
    assert np.all(run_assign(eng, P, R, np.full(len(R), -1)) == -1)
    # the rows of the 4096-row case against themselves: every row finds itself
    if nfree == 3:
        _, R, kw, _ = LINK_CASES[-1]
        labels, _, _ = modes.link_host(R, **kw)
        assert np.array_equal(run_assign(eng, R[::7], R, labels), labels[::7])
        rng = np.random.default_rng(2)
        P = rng.uniform(0, 1, (1000, 3))
        assert np.array_equal(run_assign(eng, P, R, labels), modes.assign_host(P, R, labels))


def test_rows_against_the_host_statement(eng):
    import torch
    from pyratbay_amd import _capi, modes
    from pyratbay_amd._device import _ptr, _stream
    rng = np.random.default_rng(3)
    for n, share, cap in ((1, 1.0, 4), (255, 0.5, 300), (256, 0.0, 8), (257, 0.3, 40),
                          (70000, 0.05, 4096), (70000, 0.5, 4096)):
        counts = (rng.uniform(0, 1, n) < share) * rng.integers(1, 9, n)
        want = modes.rows_host(counts)
        rows, nrows = int_tensor((cap + 1,), 'int64'), int_tensor((2,), 'int64')
        counts_d = eng.dev(counts, torch.int64)
        _capi.call('pb_modes_rows', _ptr(rows), _ptr(nrows), _ptr(counts_d), n, cap, _stream())
        torch.cuda.synchronize()
        assert int(nrows[0]) == len(want) and int(nrows[1]) == -77 and int(rows[cap]) == -77
        kept = min(len(want), cap)
        assert np.array_equal(host(rows[:kept]), want[:kept])
        assert np.all(host(rows[kept:]) == -77)


def run_evidence(eng, logw, logl, mode, nmodes, ln_z):
    import torch
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    outs = [nan_tensor((nmodes + 1,)) for _ in range(3)]
    outs[0][nmodes] = outs[1][nmodes] = outs[2][nmodes] = 7.0
    logw_d, logl_d, mode_d = eng.dev(logw), eng.dev(logl), dev_i32(eng, mode)
    ln_z_d = eng.dev(np.array([ln_z]))
    _capi.call('pb_modes_evidence', *(_ptr(o) for o in outs), _ptr(logw_d), _ptr(logl_d),
               _ptr(mode_d), _ptr(ln_z_d), len(logw), nmodes, _stream())
    torch.cuda.synchronize()
    assert all(float(o[nmodes]) == 7.0 for o in outs)
    return [host(o[:nmodes]) for o in outs]


@pytest.mark.parametrize('ndead,nlive', mc.nc.FINISH_SHAPES)
def test_evidence_against_the_host_statement(eng, ndead, nlive):
    from pyratbay_amd import modes, nested
    dead_logl, dead_logw, live_logl, ln_x = mc.nc.finish_case(ndead, nlive, ndead + nlive)
    fin = nested.finish_host(dead_logl, dead_logw, live_logl, ln_x)
    N = len(fin.logw)
    mode = np.random.default_rng(N).integers(-1, 3, N).astype(np.int32)
    want = modes.evidence_host(fin.logw, fin.logl, mode, 4, fin.ln_z)
    got = run_evidence(eng, fin.logw, fin.logl, mode, 4, fin.ln_z)
    for g, w in zip(got, want):
        finite = np.isfinite(w)
        print(f'({ndead}, {nlive}): device - host {g[finite] - w[finite]}')
        assert np.array_equal(g[~finite], w[~finite], equal_nan=True), (g, w)
        assert np.all(np.abs(g[finite] - w[finite]) <= 1e-12 * np.maximum(np.abs(w[finite]), 1.0))
    # the mode nobody is in: -inf, NaN, 0
    assert got[0][3] == -np.inf and np.isnan(got[1][3]) and got[2][3] == 0.0


def test_refusals(eng):
    from pyratbay_amd import _capi
    from pyratbay_amd._device import _ptr, _stream
    PbError = _capi.PbError
    f, i = nan_tensor((4200 * 3,)), int_tensor((4200 * 140,), 'int64', 0)
    p, q, s = _ptr(f), _ptr(i), _stream()

    def link(*tail, ptrs=None):
        _capi.call('pb_modes_link', *(ptrs or [q, q, p, p, q, p]), *tail, s)
    # (n, nfree, knn, link, min_mode, max_modes)
    with pytest.raises(PbError, match='pb_modes_link: 1 rows: at least 2'):
        link(1, 3, 10, 1.0, 8, 16)
    with pytest.raises(PbError, match='pb_modes_link: 4097 rows: 1 to 4096'):
        link(4097, 3, 10, 1.0, 8, 16)
    with pytest.raises(PbError, match='pb_modes_link: 129 free parameters: 1 to 128'):
        link(10, 129, 10, 1.0, 8, 16)
    for knn in (0, 33):
        with pytest.raises(PbError, match=f'pb_modes_link: knn = {knn}: 1 to 32'):
            link(10, 3, knn, 1.0, 8, 16)
    with pytest.raises(PbError, match='pb_modes_link: max_modes = 0: at least 1'):
        link(10, 3, 10, 1.0, 8, 0)
    for k in range(6):
        ptrs = [q, q, p, p, q, p]
        ptrs[k] = None
        with pytest.raises(PbError, match='pb_modes_link: null pointer'):
            link(10, 3, 10, 1.0, 8, 16, ptrs=ptrs)
    with pytest.raises(PbError, match='pb_modes_assign: 4097 rows'):
        _capi.call('pb_modes_assign', q, p, p, q, 5, 4097, 3, s)
    with pytest.raises(PbError, match='pb_modes_assign: 0 free parameters'):
        _capi.call('pb_modes_assign', q, p, p, q, 5, 10, 0, s)
    with pytest.raises(PbError, match='pb_modes_assign: bad shape'):
        _capi.call('pb_modes_assign', q, p, p, q, -1, 10, 3, s)
    with pytest.raises(PbError, match='pb_modes_assign: null pointer'):
        _capi.call('pb_modes_assign', q, p, None, q, 5, 10, 3, s)
    with pytest.raises(PbError, match='pb_modes_sqdist: null pointer'):
        _capi.call('pb_modes_sqdist', None, p, p, 5, 10, 3, s)
    with pytest.raises(PbError, match='pb_modes_sqdist: 0 rows'):
        _capi.call('pb_modes_sqdist', p, p, p, 5, 0, 3, s)
    with pytest.raises(PbError, match='pb_modes_rows: bad shape'):
        _capi.call('pb_modes_rows', q, q, q, 0, 5, s)
    with pytest.raises(PbError, match='pb_modes_rows: null pointer'):
        _capi.call('pb_modes_rows', q, None, q, 5, 5, s)
    with pytest.raises(PbError, match='pb_modes_evidence: bad shape'):
        _capi.call('pb_modes_evidence', p, p, p, p, p, q, p, 0, 2, s)
    with pytest.raises(PbError, match='pb_modes_evidence: null pointer'):
        _capi.call('pb_modes_evidence', p, p, p, p, p, q, None, 5, 2, s)
    # no points, no modes: nothing launched
    _capi.call('pb_modes_assign', q, p, p, q, 0, 10, 3, s)
    _capi.call('pb_modes_evidence', p, p, p, p, p, q, p, 5, 0, s)


# -------------------------------------------------------------------------------------------------
# NestedSampler.modes on the two-mode target
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', list(mc.FORMS))
def test_modes_of_a_run_on_the_two_mode_target(eng, form):
    """nlive 512, batch 128, nsteps 30, dlogz 0.01 at seed 0 on the device, then modes(): the
    bits of modes_host applied to the read-back state of the same run (the device's ln w, ln L,
    cdf and ln Z); two modes within the bounds committed for the host statement; two
    read-backs."""
    import torch
    from pyratbay_amd import modes
    log_like, prior_transform = mc.target_torch(form)
    ns = eng.NestedSampler(log_like, prior_transform, mc.NFREE, mc.NLIVE, batch=mc.BATCH,
                           nsteps=mc.NSTEPS, seed=0).start()
    ns.run_until(mc.DLOGZ, check_every=1, max_iter=mc.MAX_ITER)
    assert ns.it < mc.MAX_ITER
    before = {name: getattr(ns, name).clone() for name in ('live_u', 'live_logl', 'state')}
    found = []
    assert no_read_back(lambda: found.append(ns.modes())) == ['item', 'item']
    md = found[0]
    for name, was in before.items():
        assert torch.equal(getattr(ns, name), was), name
    out, logw, logl, cdf = ns._finish()
    fin = types.SimpleNamespace(logw=host(logw), logl=host(logl), cdf=host(cdf),
                                ln_z=float(out[0]))
    cube = host(ns._cube())
    want = modes.modes_host(cube, fin, ns.seed)
    assert md.nmodes == want.nmodes == 2
    assert md.mode.dtype == torch.int32 and md.labels.dtype == torch.int32
    assert np.array_equal(host(md.rows), want.rows)
    assert np.array_equal(host(md.labels), want.labels)
    assert bits(float(md.ell2)) == bits(want.ell2)
    assert np.array_equal(host(md.mode), want.mode)
    for name in ('ln_z', 'info', 'fraction'):
        got, w = host(getattr(md, name)), getattr(want, name)
        print(f'{form}: {name} device - host {got - w}, {int(np.sum(bits(got) != bits(w)))} of 2 '
              'differ in bits')
        assert got.shape == (2,) and np.array_equal(bits(got), bits(w))
    assert abs(np.logaddexp(*host(md.ln_z)) - fin.ln_z) <= 1e-12
    theta = host(prior_transform(ns._cube()))
    got = types.SimpleNamespace(nmodes=2, mode=host(md.mode), ln_z=host(md.ln_z))
    err, mass = mc.mode_figures(form, theta, fin.logw, fin.ln_z, got)
    print(f'{form}: {ns.it} iterations, {len(want.rows)} rows, ln Z - closed form '
          f'{fin.ln_z - mc.LN_Z:+.4f}, local {err}, misassigned mass {mass:.2e}')
    assert np.all(np.abs(err) <= mc.BOUND_LOCAL[form]) and mass <= mc.BOUND_MASS
    # other keywords reach the kernels: a link length of 20 merges everything
    one = ns.modes(nsamples=500, knn=3, link=20.0, min_mode=2, max_modes=4)
    want = modes.modes_host(cube, fin, ns.seed, nsamples=500, knn=3, link=20.0, min_mode=2,
                            max_modes=4)
    assert one.nmodes == want.nmodes == 1 and np.array_equal(host(one.rows), want.rows)
    assert np.array_equal(host(one.mode), want.mode) and bits(float(one.ell2)) == bits(want.ell2)
    # unique(mode=): the rows of unique(), split
    theta_all, counts_all = ns.unique()
    again, counts_again = ns.unique(mode=None)
    assert torch.equal(theta_all, again) and torch.equal(counts_all, counts_again)
    parts = [ns.unique(mode=c) for c in range(2)]
    assert sum(int(c.sum()) for _, c in parts) == int(counts_all.sum())
    assert sum(t.shape[0] for t, _ in parts) == theta_all.shape[0]
    both = torch.cat([t for t, _ in parts])
    assert torch.equal(both[torch.argsort(both[:, 0])], theta_all[torch.argsort(theta_all[:, 0])])
    signs = sorted(float(torch.sign(torch.median(t[:, 0]))) for t, _ in parts)
    assert signs == [-1.0, 1.0]
    for bad in (2, -1, 0.5):
        with pytest.raises(ValueError, match='the run has the modes 0 to 1'):
            ns.unique(mode=bad)
    with pytest.raises(ValueError, match='knn = 40'):
        ns.modes(knn=40)


def test_modes_of_a_run_that_has_not_begun(eng):
    """No dead point yet: the live points alone, one mode."""
    log_like, prior_transform = mc.target_torch('equal')
    ns = eng.NestedSampler(log_like, prior_transform, mc.NFREE, 64, batch=16, nsteps=8).start()
    md = ns.modes(link=20.0)
    assert md.nmodes == 1 and md.mode.shape == (64,) and bool((md.mode == 0).all())
    assert float(md.fraction[0]) == pytest.approx(1.0, abs=1e-12)


# -------------------------------------------------------------------------------------------------
# Retrieval.summary(mode=)
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def retrieval(eng, golden):
    return sc.emission_retrieval(eng, golden)


def test_retrieval_summary_of_a_mode(eng, retrieval):
    """test_gpu_nested's smallest retrieval: 32 live points, batches of 8, 4 steps, 6 iterations."""
    import torch
    ret = retrieval
    ns = ret.nested(nlive=32, seed=5, dlogz=None, batch=8, nsteps=4)
    ns.run(6)
    md = ns.modes()
    assert md.nmodes >= 1 and md.mode.shape == (80,)
    theta_all, counts_all = ns.unique()
    again, counts_again = ns.unique(mode=None)
    assert torch.equal(theta_all, again) and torch.equal(counts_all, counts_again)
    parts = [ns.unique(mode=c) for c in range(md.nmodes)]
    assert sum(int(c.sum()) for _, c in parts) == int(counts_all.sum()) == 80
    assert sum(t.shape[0] for t, _ in parts) == theta_all.shape[0]
    assert all(t.shape[1] == ret.nfree for t, _ in parts)
    whole = ret.summary(ns)
    same = ret.summary(ns, mode=None)
    assert torch.equal(whole.bands[0], same.bands[0])
    one = ret.summary(ns, mode=0)
    assert int(one.n_rejected) == 0 and bool(torch.isfinite(one.bands[0]).all())
    if md.nmodes == 1:
        assert torch.equal(one.bands[0], whole.bands[0])
    with pytest.raises(ValueError, match=f'the run has the modes 0 to {md.nmodes - 1}'):
        ret.summary(ns, mode=md.nmodes)
    with pytest.raises(ValueError, match='a DEMC has no modes'):
        ret.summary(types.new_class('DEMC')(), mode=0)
