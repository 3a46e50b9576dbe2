"""The posterior modes of a finished nested-sampling run: which mode every stored point belongs
to, and per mode a local evidence, its information and its share of the evidence -- what
MultiNest's multimodal run gives the reference's users.  The run itself does not cluster
(nested.py); the decomposition is computed afterwards from the stored points, keeps no state, and
can be taken at any time.  The NumPy statements here (sqdist_host, link_host, assign_host,
evidence_host, modes_host) ARE the specification: the kernels of csrc/pb_modes.hip are tested
against them, and they are tested on a two-mode target whose local evidences are known in closed
form (tests/modes_cases.py, profiles/modes.md).

Everything works in the unit cube, on the rows NestedSampler._cube() returns: the dead points in
the order they died, then the live points.  Those are finite by construction (a proposal outside
the cube is never stored), so no statement here has a rule for NaN.

    rows     nsamples draws of the posterior (nested.resample_host); the rows something fell on,
             ascending: at most MAX_LIVE, and they sit where the posterior mass is, so that a mode
             which dies out before the run ends is still found.
    link     single linkage at the scale of the rows' own spacing: ell2 = link^2 times the largest
             squared distance from a row to its k-th nearest other row; rows closer than that are
             linked, and the components of the links, by size, are the modes.
    assign   every stored point takes the mode of its nearest row among the rows that have one.
    evidence finish_host's sums over each mode's points.

No error bar is given for a local evidence: the share of the live points between separated modes
carries sampling noise that sqrt(H / nlive) does not cover.  profiles/modes.md has the measured
scatter over 20 seeds."""
import types

import numpy as np

from . import nested
from ._capi import constant
from .nested import FINISH_CHUNKS, MAX_LIVE, MAX_PARAMS

MAX_KNN = constant('PB_MODES_MAX_KNN')      # a row's running list of nearest rows


def default_min_mode(nfree):
    return max(int(nfree) + 1, 8)


def sqdist_host(A, B):
    """A[Na, nfree], B[Nb, nfree] -> d2[Na, Nb]: d2 = 0, then for p = 0 .. nfree - 1 in order
    t = A[i, p] - B[j, p]; d2 = d2 + t * t, every operation rounded and none fused.  (np.sum has
    another order of summation and is not this statement.)  The inputs are finite."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError(f'sqdist: shapes {A.shape} and {B.shape}')
    d2 = np.zeros((A.shape[0], B.shape[0]))
    for p in range(A.shape[1]):
        t = A[:, p, None] - B[None, :, p]
        d2 = d2 + t * t
    return d2


def _check_link(n, nfree, knn, max_modes):
    if not 2 <= n <= MAX_LIVE:
        raise ValueError(f'{n} rows: 2 to {MAX_LIVE}')
    if not 1 <= nfree <= MAX_PARAMS:
        raise ValueError(f'{nfree} free parameters: 1 to {MAX_PARAMS}')
    if not 1 <= int(knn) <= MAX_KNN:
        raise ValueError(f'knn = {knn}: 1 to {MAX_KNN}')
    if int(max_modes) < 1:
        raise ValueError(f'max_modes = {max_modes}: at least 1')


def components_host(linked):
    """linked[n, n] bool, symmetric -> root[n]: the smallest row index of every row's component
    (the transitive closure of the links), by minimum-label propagation to the fixed point."""
    n = linked.shape[0]
    root = np.arange(n)
    reach = linked | np.eye(n, dtype=bool)
    while True:
        new = np.where(reach, root[None, :], n).min(axis=1)
        new = new[new]                                  # (pointer jumping)
        if np.array_equal(new, root):
            return root
        root = new


def link_host(R, knn=10, link=1.0, min_mode=None, max_modes=16):
    """R[n, nfree], finite, 2 <= n <= 4096, 1 <= knn <= 32, nfree <= 128 -> (labels[n] int32,
    nmodes, ell2).  With d2 = sqdist_host(R, R) and k = min(knn, n - 1): dk[i] is the k-th
    smallest of the n - 1 values d2[i, j != i] (duplicates count), ell2 = (link * link) *
    max_i dk[i]; rows i != j are linked iff d2[i, j] <= ell2, and the components are the
    transitive closure of the links.  In the canonical order -- by size descending, ties to the
    component with the smallest row index -- the first max_modes components with at least
    min_mode rows (default max(nfree + 1, 8)) get the labels 0, 1, ...; every other row gets -1
    ("loose").  The largest component is mode 0 whatever its size, so nmodes >= 1.  The result
    depends on no traversal order.

    The rule is conservative: one far outlier raises ell2 and merges modes; it never splits
    one."""
    R = np.asarray(R, dtype=np.float64)
    n, nfree = R.shape
    _check_link(n, nfree, knn, max_modes)
    min_mode = default_min_mode(nfree) if min_mode is None else int(min_mode)
    k = min(int(knn), n - 1)
    d2 = sqdist_host(R, R)
    others = d2.copy()
    others[np.arange(n), np.arange(n)] = np.inf
    dk = np.partition(others, k - 1, axis=1)[:, k - 1]
    ell2 = float((float(link) * float(link)) * np.max(dk))
    linked = d2 <= ell2
    linked[np.arange(n), np.arange(n)] = False
    root = components_host(linked)
    size = np.bincount(root, minlength=n)
    roots = np.where(size > 0)[0]
    order = roots[np.lexsort((roots, -size[roots]))]
    label_of = np.full(n, -1, dtype=np.int32)
    nmodes = 0
    for q, r in enumerate(order):
        if q == 0 or (size[r] >= min_mode and q < int(max_modes)):
            label_of[r] = q
            nmodes = q + 1
    return label_of[root].astype(np.int32), nmodes, ell2


def assign_host(P, R, labels, chunk=4096):
    """P[N, nfree], R[n, nfree], labels[n] -> mode[N] int32: the label of the row with the
    smallest sqdist_host(P, R) among the rows with labels >= 0, ties to the lower row index (the
    lexicographic minimum over (d2, row), which no tiling changes).  Without a single labelled
    row every point gets -1.  The inputs are finite."""
    P = np.asarray(P, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int32)
    has = np.where(labels >= 0)[0]
    mode = np.full(P.shape[0], -1, dtype=np.int32)
    if len(has) == 0:
        return mode
    Rm = R[has]
    for lo in range(0, P.shape[0], int(chunk)):
        d2 = sqdist_host(P[lo:lo + chunk], Rm)
        mode[lo:lo + chunk] = labels[has[np.argmin(d2, axis=1)]]
    return mode


def evidence_host(logw, logl, mode, nmodes, ln_z):
    """logw[N], logl[N], mode[N], the global ln Z -> (ln_z_m, info_m, fraction_m), each [nmodes]:
    finish_host's formulae on each mode's entries.  m = the largest ln w of the mode,
    e = exp(ln w - m) inside the mode where ln w > -inf and 0 elsewhere, S = sum e,
    ln Z_m = m + ln S, H_m = (sum e ln L over e > 0) / S - ln Z_m, fraction_m = exp(ln Z_m - ln Z);
    the sums as nested._chunked_cumsum over the full-length masked arrays, pb_nested_finish's
    order.  A mode without weight has ln Z_m = -inf, fraction 0 and H_m NaN."""
    logw = np.asarray(logw, dtype=np.float64)
    logl = np.asarray(logl, dtype=np.float64)
    mode = np.asarray(mode)
    ln_z_m, info_m, fraction_m = (np.empty(int(nmodes)) for _ in range(3))
    with np.errstate(all='ignore'):
        for c in range(int(nmodes)):
            member = (mode == c) & (logw > -np.inf)
            m = np.fmax.reduce(np.where(member, logw, -np.inf), initial=-np.inf)
            e = np.where(member, np.exp(logw - m), 0.0)
            _, S = nested._chunked_cumsum(e, FINISH_CHUNKS)
            _, hsum = nested._chunked_cumsum(np.where(e > 0.0, e * logl, 0.0), FINISH_CHUNKS)
            S, hsum = np.float64(S), np.float64(hsum)
            ln_z_m[c] = m + np.log(S)
            info_m[c] = hsum / S - ln_z_m[c]
            fraction_m[c] = np.exp(ln_z_m[c] - ln_z)
    return ln_z_m, info_m, fraction_m


def rows_host(counts):
    """The indices with counts > 0, ascending."""
    return np.nonzero(np.asarray(counts) > 0)[0]


def modes_host(cube, fin, seed, nsamples=4096, **link_kw):
    """cube[N, nfree] (the dead points, then the live ones), fin (finish_host's namespace: logw,
    logl, cdf, ln_z) and the sampler's seed -> a namespace of nmodes, mode[N], ln_z[nmodes],
    info[nmodes], fraction[nmodes], rows, labels, ell2.  counts = resample_host(fin.cdf,
    min(N, nsamples), seed); rows = the indices with counts > 0, ascending; link_host(cube[rows]),
    assign_host(cube, cube[rows], labels), evidence_host.  With fewer than 2 rows everything is
    mode 0 (labels 0, ell2 0)."""
    cube = np.asarray(cube, dtype=np.float64)
    N = cube.shape[0]
    counts = nested.resample_host(fin.cdf, min(N, int(nsamples)), seed)
    rows = rows_host(counts)
    if len(rows) > MAX_LIVE:
        raise ValueError(f'{len(rows)} rows: at most {MAX_LIVE} (nsamples = {nsamples})')
    if len(rows) < 2:
        labels, nmodes, ell2 = np.zeros(len(rows), np.int32), 1, 0.0
        mode = np.zeros(N, np.int32)
    else:
        labels, nmodes, ell2 = link_host(cube[rows], **link_kw)
        mode = assign_host(cube, cube[rows], labels)
    ln_z_m, info_m, fraction_m = evidence_host(fin.logw, fin.logl, mode, nmodes, fin.ln_z)
    return types.SimpleNamespace(nmodes=nmodes, mode=mode, ln_z=ln_z_m, info=info_m,
                                 fraction=fraction_m, rows=rows, labels=labels, ell2=ell2)
