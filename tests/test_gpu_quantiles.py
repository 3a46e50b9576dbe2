"""pb_weighted_quantiles (csrc/pb_quantiles.hip) at the kernel boundary, on dirty memory: `out`
and `work` are pre-filled with NaN, the columns have ld > n with NaN in the padding.  The kernel
is an exact selection plus NumPy's three-operation lerp, so every comparison is for EQUAL VALUES
(np.array_equal; NaN = NaN where NumPy's own lerp makes one of inf - inf; -0.0 = +0.0, which
np.sort does not order either): against posterior.weighted_quantiles_host, the NumPy statement of
the kernel, and against np.percentile of the real expansion where N is small."""
import numpy as np
import pytest

from pyratbay_amd import posterior as post

pytestmark = pytest.mark.gpu

Q5 = post.QUANTILES
Q_ALL = Q5 + [0.0, 1.0, 0.25]
BLOCK = 512                      # threads of a workgroup; a pass takes 8 x BLOCK rows per sweep


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def resident_rows():
    from pyratbay_amd import _capi
    return int(_capi.lib().pb_weighted_quantiles_resident_rows())


def run(eng, values, counts, q, pad=3, total=None):
    """values[n, ncol] (host, samples first) through the C entry -> out[nq, ncol] (host)."""
    import torch
    from pyratbay_amd import _capi
    values = np.asarray(values, float)
    n, ncol = values.shape
    counts = np.asarray(counts, np.int64)
    total = int(counts[counts > 0].sum()) if total is None else total
    lo, hi, gamma = post.quantile_ranks(total, q)
    ld = n + pad
    store = torch.full((max(ncol, 1), ld), float('nan'), dtype=torch.float64, device='cuda')
    if ncol:
        store[:ncol, :n] = eng.dev(np.ascontiguousarray(values.T))
    out = torch.full((len(gamma), max(ncol, 1)), float('nan'), dtype=torch.float64, device='cuda')
    need = _capi.lib().pb_weighted_quantiles_work_doubles(n, ncol, len(gamma))
    work = torch.full((max(int(need), 8),), float('nan'), dtype=torch.float64, device='cuda')
    # (named: a temporary's memory would be handed to the next upload)
    counts_d, lo_d, hi_d = (eng.dev(x, torch.int64) for x in (counts, lo, hi))
    gamma_d = eng.dev(gamma)
    _capi.call('pb_weighted_quantiles', out.data_ptr(), store.data_ptr(), ld,
               counts_d.data_ptr(), n, ncol, lo_d.data_ptr(), hi_d.data_ptr(),
               gamma_d.data_ptr(), len(gamma), work.data_ptr(),
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(work).all()) and bool(torch.isnan(store[:, n:]).all())
    return out.cpu().numpy()[:, :ncol]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check(eng, values, counts, q=Q_ALL, expand=True):
    values = np.asarray(values, float)
    got = run(eng, values, counts, q)
    with np.errstate(invalid='ignore'):
        want = post.weighted_quantiles_host(values, counts, q)
        assert same(got, want), (got, want)
        if expand:
            full = values[np.repeat(np.arange(len(counts)), counts)]
            assert same(got, np.percentile(full, 100 * np.array(q), axis=0))
    return got


@pytest.mark.parametrize('counts', [[1], [7], [1, 1], [5, 1], [1, 1, 1], [5, 1, 2]])
def test_tiny_samples(eng, counts):
    rng = np.random.default_rng(len(counts) + sum(counts))
    check(eng, rng.normal(size=(len(counts), 7)), counts)


@pytest.mark.parametrize('n', [63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 8 * BLOCK - 1, 8 * BLOCK,
                               8 * BLOCK + 1])
@pytest.mark.parametrize('ncol', [1, 7, 130])
def test_sizes_around_the_wavefront_and_the_workgroup(eng, n, ncol):
    """Normal values of mixed sign (every radix pass from the sign down), counts 0 ... 5."""
    rng = np.random.default_rng(1000 * ncol + n)
    counts = rng.integers(0, 6, n)
    counts[rng.integers(0, n)] = 2
    check(eng, rng.normal(size=(n, ncol)) * 10.0**rng.uniform(-3, 3, ncol), counts)


def test_both_regimes_at_the_boundary(eng):
    """n = pb_weighted_quantiles_resident_rows() (the column staged in LDS) and + 1 (every pass
    re-reads it), the boundary read from the library: the same 7 columns, one row more."""
    import torch
    r = resident_rows()
    assert r >= 1
    rng = np.random.default_rng(8)
    values = rng.normal(1.0e-3, 1.0e-5, (r + 1, 7))       # spectra-like: shared leading bytes
    values[:, 5] = rng.integers(0, 5, r + 1)              # ties
    values[:, 6] *= rng.choice([-1.0, 1.0], r + 1)
    counts = rng.integers(0, 4, r + 1)
    counts[-1] = 3
    a = check(eng, values[:r], counts[:r], expand=False)
    b = check(eng, values, counts, expand=False)
    assert not np.array_equal(a, b)
    torch.cuda.synchronize()


def test_ties_special_values_and_the_last_pass(eng):
    rng = np.random.default_rng(4)
    n = 200
    base = rng.uniform(1.0, 2.0, n)
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.5e-310, -2.5e-310, 2.3e-308, -1.0, 1.0])
    cols = [np.full(n, 3.25),                                          # all equal: no pass
            np.array([-2.5, -1e-3, 0.0, 0.7, 3.25e4])[rng.integers(0, 5, n)],
            tiny[rng.integers(0, len(tiny), n)],                       # +-0.0 and denormals
            np.where(rng.integers(0, 2, n) == 1, np.nextafter(1.5, 2.0), 1.5),   # the lowest bit
            np.where(rng.integers(0, 2, n) == 1, np.nextafter(base, 4.0), base),
            -base]
    counts = rng.integers(0, 6, n)
    counts[0] = 1
    check(eng, np.stack(cols, axis=1), counts)


def test_rows_that_do_not_exist(eng):
    """Count 0 on the smallest and on the largest value of every column (and on others): they are
    in no quantile, q = 0 and 1 included; a column with no row at all gets NaN."""
    rng = np.random.default_rng(6)
    n = 70
    values = rng.normal(size=(n, 7))
    counts = rng.integers(0, 4, n)
    counts[:8] = 1
    values[8] = -100.0
    values[9] = 100.0
    counts[8] = counts[9] = 0
    got = check(eng, values, counts)
    keep = counts > 0
    assert np.array_equal(got[Q_ALL.index(0.0)], values[keep].min(axis=0))
    assert np.array_equal(got[Q_ALL.index(1.0)], values[keep].max(axis=0))
    none = run(eng, values, np.zeros(n, np.int64), Q5, total=1)
    assert none.shape == (5, 7) and np.all(np.isnan(none))


def test_infinity_at_the_top(eng):
    """A +inf with a non-zero count: the quantiles below it are finite; the one that selects it is
    what NumPy's lerp makes of inf - inf (np.percentile returns NaN there, and so does this)."""
    values = np.array([[1.0, 4.0], [np.inf, 2.0], [3.0, np.inf], [2.0, 8.0]])
    got = check(eng, values, [2, 1, 3, 2], q=[0.0, 0.5, 1.0])
    assert np.array_equal(got[0], [1.0, 2.0]) and np.isfinite(got[1, 0]) and np.isnan(got[2, 0])


def test_gamma_zero_and_half(eng):
    """N = 5, q = 0.5: v = 2, gamma = 0 exactly; N = 4, q = 0.5: gamma = 0.5 (the branch b - d
    (1 - t)); N = 4, q = 0.97725: gamma above 0.5."""
    rng = np.random.default_rng(9)
    values = rng.normal(size=(3, 9))
    assert post.quantile_ranks(5, [0.5])[2][0] == 0.0
    assert post.quantile_ranks(4, [0.5])[2][0] == 0.5
    assert post.quantile_ranks(4, [0.97725])[2][0] > 0.5
    check(eng, values, [2, 2, 1], q=[0.5])
    check(eng, values, [1, 2, 1], q=[0.5, 0.97725])


def test_more_quantiles_than_one_batch(eng):
    """13 quantiles: the kernel resolves six at a time."""
    rng = np.random.default_rng(10)
    counts = rng.integers(0, 5, 300)
    counts[3] = 1
    check(eng, rng.normal(size=(300, 5)), counts, q=list(np.linspace(0.0, 1.0, 13)))


def test_counts_past_2_to_the_31(eng):
    """Counts near 1e10 each: against the host statement only (no expansion)."""
    rng = np.random.default_rng(11)
    n = 50
    counts = 10**10 + rng.integers(0, 10**6, n)
    counts[7] = 0
    assert counts.sum() > 2**31
    check(eng, rng.normal(size=(n, 7)), counts, expand=False)


def test_two_runs_have_equal_bits(eng):
    rng = np.random.default_rng(12)
    values = rng.normal(size=(3000, 130))
    counts = rng.integers(0, 6, 3000)
    a, b = run(eng, values, counts, Q5), run(eng, values, counts, Q5)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_no_columns_and_refused_arguments(eng):
    """ncol = 0 succeeds and leaves `out` alone; n < 1, nq < 1, ncol < 0, ld < n and a null
    pointer return the error before any launch (`out` keeps its NaNs)."""
    import torch
    from pyratbay_amd import _capi
    n, ncol, nq = 10, 3, 2
    store = torch.ones((ncol, n), dtype=torch.float64, device='cuda')
    counts = torch.ones(n, dtype=torch.int64, device='cuda')
    lo = torch.zeros(nq, dtype=torch.int64, device='cuda')
    gamma = torch.zeros(nq, dtype=torch.float64, device='cuda')
    out = torch.full((nq, ncol), float('nan'), dtype=torch.float64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(out=out.data_ptr(), values=store.data_ptr(), ld=n, counts=counts.data_ptr(), n=n,
                 ncol=ncol, lo=lo.data_ptr(), hi=lo.data_ptr(), gamma=gamma.data_ptr(), nq=nq)
        a.update(kw)
        return _capi.call('pb_weighted_quantiles', a['out'], a['values'], a['ld'], a['counts'],
                          a['n'], a['ncol'], a['lo'], a['hi'], a['gamma'], a['nq'], None, stream)

    assert call(ncol=0) == _capi.PB_OK
    for bad in (dict(n=0), dict(nq=0), dict(ncol=-1), dict(ld=n - 1), dict(out=None),
                dict(values=None), dict(counts=None), dict(lo=None), dict(hi=None),
                dict(gamma=None)):
        with pytest.raises(_capi.PbError, match='pb_weighted_quantiles'):
            call(**bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == _capi.PB_OK
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())


def test_front_end_shapes(eng):
    """posterior.weighted_quantiles: any leading shape [..., n] is flattened to columns, a 2-D
    view with a row stride above n is taken as it is, counts from the host or the device."""
    import torch
    rng = np.random.default_rng(13)
    values = rng.normal(size=(4, 6, 33))
    counts = rng.integers(0, 4, 33)
    counts[0] = 1
    want = post.weighted_quantiles_host(np.moveaxis(values, -1, 0), counts, Q5)
    got = post.weighted_quantiles(eng.dev(values), counts, Q5)
    assert got.shape == (5, 4, 6) and np.array_equal(got.cpu().numpy(), want)
    wide = torch.full((24, 40), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :33] = eng.dev(values.reshape(24, 33))
    got2 = post.weighted_quantiles(wide[:, :33], eng.dev(counts, torch.int64), Q5)
    assert torch.equal(got2, got.reshape(5, 24))
    with pytest.raises(ValueError):
        post.weighted_quantiles(eng.dev(values), counts[:-1], Q5)
    with pytest.raises(ValueError, match='every count is zero'):
        post.weighted_quantiles(eng.dev(values), np.zeros(33, np.int64), Q5)
