"""The NumPy statements of the mode decomposition (pyratbay_amd/modes.py), which are the
specification of csrc/pb_modes.hip: against brute-force restatements on the hand-made cases of
modes_cases, and on a two-mode target whose local evidences are known in closed form (20 seeds,
two forms, profiles/modes.md)."""
import os
import types

import numpy as np
import pytest

import modes_cases as mc
from pyratbay_amd import modes, nested


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# -------------------------------------------------------------------------------------------------
# brute-force restatements
# -------------------------------------------------------------------------------------------------
def sqdist_loops(A, B):
    d2 = np.zeros((len(A), len(B)))
    for i in range(len(A)):
        for j in range(len(B)):
            s = 0.0
            for p in range(A.shape[1]):
                t = A[i, p] - B[j, p]
                s = s + t * t
            d2[i, j] = s
    return d2


def link_brute(R, knn=10, link=1.0, min_mode=None, max_modes=16):
    """link_host restated: sorted distances, union-find, a sort of (size, first row)."""
    n, nfree = R.shape
    min_mode = max(nfree + 1, 8) if min_mode is None else min_mode
    d2 = sqdist_loops(R, R) if n <= 9 else modes.sqdist_host(R, R)
    k = min(knn, n - 1)
    dk = [sorted(d2[i, j] for j in range(n) if j != i)[k - 1] for i in range(n)]
    ell2 = (link * link) * max(dk)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in zip(*np.nonzero(d2 <= ell2)):
        if i != j:
            parent[find(max(i, j))] = find(min(i, j))
    roots = [find(i) for i in range(n)]
    members = {}
    for i, r in enumerate(roots):
        members.setdefault(r, []).append(i)
    order = sorted(members.values(), key=lambda rows: (-len(rows), rows[0]))
    labels = np.full(n, -1, np.int32)
    nmodes = 0
    for q, rows in enumerate(order):
        if q == 0 or (len(rows) >= min_mode and q < max_modes):
            labels[rows] = q
            nmodes = q + 1
    return labels, nmodes, ell2, d2


def test_sqdist_is_the_left_to_right_sum():
    rng = np.random.default_rng(0)
    for na, nb, nfree in ((1, 1, 1), (3, 5, 3), (4, 2, 17), (2, 3, 128)):
        A, B = rng.uniform(0, 1, (na, nfree)), rng.uniform(0, 1, (nb, nfree))
        assert np.array_equal(bits(modes.sqdist_host(A, B)), bits(sqdist_loops(A, B)))
    # np.sum is another statement: at 128 parameters its bits differ somewhere
    A, B = rng.uniform(0, 1, (40, 128)), rng.uniform(0, 1, (40, 128))
    other = np.sum((A[:, None, :] - B[None, :, :])**2, axis=2)
    assert not np.array_equal(bits(modes.sqdist_host(A, B)), bits(other))
    with pytest.raises(ValueError, match='sqdist: shapes'):
        modes.sqdist_host(np.zeros((2, 3)), np.zeros((2, 4)))


LINK_CASES = mc.link_cases()


@pytest.mark.parametrize('kind', mc.KINDS)
def test_link_against_union_find(kind):
    seen = 0
    for name, R, kw, expect in LINK_CASES:
        if not name.startswith(kind + '-') or len(R) > 300:
            continue
        seen += 1
        assert np.all((R > 0) & (R < 1)), name
        labels, nmodes, ell2 = modes.link_host(R, **kw)
        want, want_nmodes, want_ell2, d2 = link_brute(R, **kw)
        assert labels.dtype == np.int32 and np.array_equal(labels, want), name
        assert nmodes == want_nmodes and bits(ell2) == bits(want_ell2), name
        assert nmodes >= 1 and labels.max() == nmodes - 1 and np.any(labels == 0), name
        if expect is not None:
            assert nmodes == expect, (name, nmodes, expect)
        if kind == 'equal':
            # equal sizes: the modes in the order of their first rows
            first = [np.where(labels == c)[0][0] for c in range(nmodes)]
            assert first == sorted(first) and first[0] == 0, name
            assert len(set(np.bincount(labels))) == 1, name
        if kind == 'small':
            assert np.sum(labels == -1) == 3 and np.all(labels[-3:] == -1), name
        if kind == 'many':
            assert np.sum(labels == -1) > 0 and len(set(labels)) == 4, name
        if kind == 'repeated':
            off = d2[~np.eye(len(R), dtype=bool)]
            assert np.sum(off == 0.0) >= 2 * (len(R) // 2), name
            if len(R) % 2 == 0:
                assert ell2 == 0.0 and nmodes == len(R) // 2, name
        if kind == 'lattice':
            off = d2[~np.eye(len(R), dtype=bool)]
            assert np.sum(off == ell2) >= 4 and nmodes == 2, name
    assert seen >= 12


def test_link_4096_rows():
    name, R, kw, expect = LINK_CASES[-1]
    assert R.shape == (4096, 3)
    labels, nmodes, ell2 = modes.link_host(R, **kw)
    assert nmodes == expect == 2
    assert np.all(labels[:2731] == 0) and np.all(labels[2731:] == 1)


def test_an_outlier_merges_and_never_splits():
    rng = np.random.default_rng(8)
    R = np.concatenate((0.4 + rng.uniform(-0.05, 0.05, (40, 3)),
                        0.6 + rng.uniform(-0.05, 0.05, (24, 3))))
    labels, nmodes, ell2 = modes.link_host(R)
    assert nmodes == 2 and np.all(labels[:40] == 0) and np.all(labels[40:] == 1)
    R[0] = 0.999
    merged, nmodes, wide = modes.link_host(R)
    assert nmodes == 1 and wide > ell2 and np.all(merged == 0)


def test_link_refusals():
    R = np.full((3, 2), 0.5)
    for kw, match in ((dict(knn=0), 'knn = 0: 1 to 32'), (dict(knn=33), 'knn = 33'),
                      (dict(max_modes=0), 'max_modes = 0')):
        with pytest.raises(ValueError, match=match):
            modes.link_host(R, **kw)
    with pytest.raises(ValueError, match='1 rows: 2 to 4096'):
        modes.link_host(R[:1])
    with pytest.raises(ValueError, match='4097 rows'):
        modes.link_host(np.zeros((4097, 1)))
    with pytest.raises(ValueError, match='129 free parameters'):
        modes.link_host(np.zeros((3, 129)))


@pytest.mark.parametrize('nfree', mc.LINK_NFREES)
def test_assign_against_a_double_loop(nfree):
    for variant in ('modes', 'loose'):
        for N in mc.ASSIGN_NS:
            P, R, labels = mc.assign_case(N, nfree, variant)
            got = modes.assign_host(P, R, labels, chunk=64)
            d2 = modes.sqdist_host(P, R)
            want = np.empty(N, np.int32)
            for i in range(N):
                best = None
                for j in range(len(R)):
                    if labels[j] >= 0 and (best is None or d2[i, j] < d2[i, best]):
                        best = j
                want[i] = labels[best]
            assert got.dtype == np.int32 and np.array_equal(got, want), (variant, N)
            assert np.array_equal(got, modes.assign_host(P, R, labels, chunk=1000))
            if variant == 'loose':
                assert np.all(got == 0) and np.sum(labels == -1) > 0
            else:
                # P[0] is equidistant from rows of both modes: the lower row wins
                near = np.where(d2[0] == d2[0].min())[0]
                assert set(labels[near]) == {0, 1} and got[0] == labels[near[0]]
            if N == 1000 and variant == 'modes':
                assert set(got) == {0, 1}
    assert np.all(modes.assign_host(P, R, np.full(len(R), -1)) == -1)


def test_evidence_against_direct_sums():
    rng = np.random.default_rng(5)
    dead_logl, dead_logw, live_logl, ln_x = mc.nc.finish_case(5120, 512, 3)
    fin = nested.finish_host(dead_logl, dead_logw, live_logl, ln_x)
    N = len(fin.logw)
    mode = rng.integers(-1, 3, N).astype(np.int32)
    mode[fin.logw == -np.inf] = 0
    ln_z_m, info_m, fraction_m = modes.evidence_host(fin.logw, fin.logl, mode, 4, fin.ln_z)
    for c in range(3):
        member = (mode == c) & (fin.logw > -np.inf)
        z = np.logaddexp.reduce(fin.logw[member])
        p = np.exp(fin.logw[member] - z)
        assert ln_z_m[c] == pytest.approx(z, rel=1e-13)
        assert info_m[c] == pytest.approx(np.sum(p * fin.logl[member]) - z, rel=1e-11)
        assert fraction_m[c] == pytest.approx(np.exp(z - fin.ln_z), rel=1e-12)
    # a mode without a row
    assert ln_z_m[3] == -np.inf and fraction_m[3] == 0.0 and np.isnan(info_m[3])
    # one mode holding everything: finish_host's own bits
    ln_z_m, info_m, fraction_m = modes.evidence_host(fin.logw, fin.logl, np.zeros(N, np.int32), 1,
                                                     fin.ln_z)
    assert bits(ln_z_m[0]) == bits(fin.ln_z) and bits(info_m[0]) == bits(fin.info)
    assert fraction_m[0] == 1.0


def test_modes_of_few_rows():
    """Fewer than 2 rows: everything is mode 0."""
    fin = types.SimpleNamespace(logw=np.array([-np.inf, 0.0, -np.inf]), logl=np.zeros(3),
                                cdf=np.array([0.0, 1.0, 1.0]), ln_z=0.0)
    md = modes.modes_host(np.full((3, 2), 0.5), fin, 1)
    assert md.nmodes == 1 and list(md.rows) == [1] and list(md.mode) == [0, 0, 0]
    assert md.ln_z[0] == 0.0 and md.fraction[0] == 1.0 and md.ell2 == 0.0


# -------------------------------------------------------------------------------------------------
# the two-mode target
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', list(mc.FORMS))
def test_local_evidences_of_the_two_mode_target(form):
    """run_host at nlive 512, batch 128, nsteps 30, dlogz 0.01 over seeds 0 - 19, then modes_host
    (the table is in profiles/modes.md).  For every seed: two modes; the per-mode rows partition
    the rows of the resample; logaddexp of the local evidences is ln Z to 1e-12; at most 1e-2 of
    the posterior mass lies across theta_0 = 0 from its mode; every local evidence within the
    committed bound of its closed form; the median of theta_0 of a mode has the sign of its
    centre.  Over the seeds: the mean of each local evidence within 3 std / sqrt(20) of the
    closed form, and the worst figures are those the bounds were made from."""
    assert mc.BOUND_LOCAL[form] <= 0.5 and mc.BOUND_LOCAL[form] == 2 * mc.WORST_LOCAL[form]
    errs, masses, straddles = [], [], 0
    for seed in mc.SEEDS:
        r = mc.run_host(form, seed)
        md, fin = r.md, r.fin
        assert r.st.remain < mc.DLOGZ and r.st.it < mc.MAX_ITER
        assert md.nmodes == 2, (seed, md.nmodes)
        assert 2 <= len(md.rows) <= nested.MAX_LIVE and np.all(np.diff(md.rows) > 0)
        assert set(md.mode) == {0, 1} and np.array_equal(md.mode[md.rows][md.labels >= 0],
                                                         md.labels[md.labels >= 0])
        assert abs(np.logaddexp(md.ln_z[0], md.ln_z[1]) - fin.ln_z) <= 1e-12
        assert abs(md.fraction.sum() - 1.0) <= 1e-12
        # unique(mode=): the counts of the one resample, split by mode
        counts = nested.resample_host(fin.cdf, len(fin.cdf), seed)
        keep = counts > 0
        parts = [np.where(keep & (md.mode == c))[0] for c in range(2)]
        assert np.array_equal(np.sort(np.concatenate(parts)), np.where(keep)[0])
        assert sum(counts[p].sum() for p in parts) == counts.sum() == len(fin.cdf)
        err, mass = mc.mode_figures(form, r.theta, fin.logw, fin.ln_z, md)
        assert np.all(np.abs(err) <= mc.BOUND_LOCAL[form]), (seed, err)
        assert mass <= mc.BOUND_MASS, (seed, mass)
        # medians as posterior_summary takes them: per mode on the mode's side, over all rows
        # wherever the larger mode is
        medians = [mc.weighted_median(r.theta[p, 0], counts[p].astype(float)) for p in parts]
        assert sorted(np.sign(medians)) == [-1.0, 1.0]
        assert all(abs(abs(m) - 5.0) < 1.0 for m in medians), medians
        both = mc.weighted_median(r.theta[keep, 0], counts[keep].astype(float))
        straddles += int(abs(abs(both) - 5.0) >= 1.0)
        errs.append(err), masses.append(mass)
    errs = np.array(errs)
    std = np.std(errs, axis=0, ddof=1)
    print(f'{form}: worst |ln Z_m - closed form| {np.max(np.abs(errs)):.5f}, mean {errs.mean(0)}, '
          f'std {std}; worst misassigned mass {max(masses):.3e}; the all-rows median of theta_0 '
          f'lies outside both modes in {straddles} seeds')
    assert np.all(np.abs(errs.mean(axis=0)) <= 3.0 * std / np.sqrt(len(mc.SEEDS)))
    np.testing.assert_allclose(np.max(np.abs(errs)), mc.WORST_LOCAL[form], atol=1e-5)
    np.testing.assert_allclose(max(masses), mc.WORST_MASS[form], rtol=1e-3)


def test_link_2_merges_the_wide_form_in_some_seeds():
    """Why the default link stays at 1: at link = 2 the wide form is one mode in some seeds."""
    merged = 0
    for seed in mc.SEEDS[:8]:
        r = mc.run_host('wide', seed)
        merged += modes.modes_host(r.cube, r.fin, seed, link=2.0).nmodes == 1
    print(f'link = 2: {merged} of 8 seeds merge')
    assert merged >= 1


def test_the_library_exports_the_entries():
    from pyratbay_amd import _capi, engine
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(os.path.dirname(here), 'include', 'pbhip.h')).read()
    for name in ('pb_modes_sqdist', 'pb_modes_link', 'pb_modes_assign', 'pb_modes_rows',
                 'pb_modes_evidence'):
        assert name in text and name in _capi.exported_names() and hasattr(_capi.lib(), name)
    assert engine.modes is modes and callable(engine.NestedSampler.modes)
    assert modes.MAX_KNN == 32 and f'#define PB_MODES_MAX_KNN {modes.MAX_KNN}' in text
    # a sampler without modes is refused before anything is launched
    with pytest.raises(ValueError, match='a DEMC has no modes'):
        engine.Retrieval.summary(None, types.new_class('DEMC')(), mode=0)
