"""The sampler of the batched retrieval loop: DEMC-zs (ter Braak & Vrugt 2008, Stat. Comput. 18,
435; the algorithm behind the reference's default `sampler = snooker`), many parallel chains whose
proposals are differences of rows of a shared history, so that one generation is one batch:

    pb_demc_propose -> log_post(prop[nw, nfree]) -> pb_demc_accept

with launches only and nothing read back (csrc/pb_sampler.hip).  The reference hands its
log-likelihood to third-party samplers that evaluate one vector per call; none of them is part of
this package and no parity with their random streams is claimed.  The NumPy statements here
(philox_host, uniforms_host, propose_host, accept_host, gelman_rubin_host, run_host) ARE the
specification: the kernels are tested against them, and they are tested for sampling a known
target.

Random numbers: Philox4x32-10, a counter-based generator, gives host and device the same words
bit for bit.  Addressing is stateless -- key = the 64-bit seed (low word, high word), counter =
(block, chain, generation, tag) with the tags TAG_PROPOSE, TAG_ACCEPT, TAG_INITIAL -- which is what
makes run(a) followed by run(b) the same as run(a + b).  A block's words (0, 1) and (2, 3) give
two uniforms u = (n + 0.5) 2^-52 with n = ((x_a >> 6) << 26) + (x_b >> 6): exact, in
[2^-53, 1 - 2^-53], and two normals by Box-Muller from those two.

The chain: sample 0 of a chain is its starting state, sample t its state after generation t
(generations count from 1, and generation t draws with g = t).  The chain store keeps a chain as
its distinct rows and how long it stayed on each: rows[nw, cap, nfree], row_logp[nw, cap],
row_gen[nw, cap] (the sample a row begins with), counts[nw, cap], nrows[nw]; an accept that finds
no room sets overflow[w] and the chain stops recording (it goes on sampling).  The history Z grows
by the nw current states after every thin_z-th generation while it has room: its capacity is
M0 + nw (capacity // thin_z) rows, fixed at the start.
"""
import types

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TAG_PROPOSE, TAG_ACCEPT, TAG_INITIAL = 0, 1, 2
MAX_GENERATIONS = 2**32
_MASK = np.uint64(0xFFFFFFFF)
_SHIFT = np.uint64(32)


# ------------------------------------------------------------------------------ random numbers
def philox_host(counter, key):
    """Philox4x32-10: counter[..., 4], key[..., 2] (32-bit words) -> [..., 4] uint32.  Ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key
    raised by (W0, W1) after each."""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] & _MASK for i in range(4))
    k0, k1 = key[..., 0] & _MASK, key[..., 1] & _MASK
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    w0, w1 = np.uint64(PHILOX_W0), np.uint64(PHILOX_W1)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> _SHIFT) ^ c1 ^ k0, p1 & _MASK, (p0 >> _SHIFT) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + w0) & _MASK, (k1 + w1) & _MASK
    out = np.broadcast_arrays(c0, c1, c2, c3)
    return np.stack(out, axis=-1).astype(np.uint32)


def block_host(seed, block, chain, generation, tag):
    """The words [..., 4] of the blocks (block, chain, generation, tag), broadcast, under seed."""
    seed = int(seed) % 2**64
    parts = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64)
                                  for a in (block, chain, generation, tag)))
    return philox_host(np.stack(parts, axis=-1), [seed & 0xFFFFFFFF, seed >> 32])


def u01_host(hi, lo):
    """Two words -> the uniform (n + 0.5) 2^-52, n = ((hi >> 6) << 26) + (lo >> 6)."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    n = ((hi >> np.uint64(6)) << np.uint64(26)) + (lo >> np.uint64(6))
    return (n.astype(np.float64) + 0.5) * 2.0**-52


def block_uniforms_host(seed, block, chain, generation, tag):
    """The two uniforms of each block."""
    x = block_host(seed, block, chain, generation, tag)
    return u01_host(x[..., 0], x[..., 1]), u01_host(x[..., 2], x[..., 3])


def index_host(u, n):
    """An index into n rows: min(floor(u n), n - 1)."""
    return np.minimum(np.floor(np.asarray(u) * float(n)).astype(np.int64), int(n) - 1)


def uniforms_host(seed, n, ncol):
    """[n, ncol]: the uniforms of the initial draw (TAG_INITIAL): row = chain slot, g = 0, block
    col // 2, even columns from words (0, 1), odd ones from words (2, 3)."""
    col = np.arange(ncol)
    ua, ub = block_uniforms_host(seed, (col // 2)[None, :], np.arange(n)[:, None], 0, TAG_INITIAL)
    return np.where((col % 2 == 0)[None, :], ua, ub)


def normals_host(seed, chains, g, nfree):
    """[len(chains), nfree]: n_f from block 3 + f // 2 of TAG_PROPOSE by Box-Muller: even f
    sqrt(-2 ln u_a) cos(2 pi u_b), odd f sqrt(-2 ln u_a) sin(2 pi u_b)."""
    f = np.arange(nfree)
    ua, ub = block_uniforms_host(seed, (3 + f // 2)[None, :], np.asarray(chains)[:, None], g,
                                 TAG_PROPOSE)
    r = np.sqrt(-2.0 * np.log(ua))
    angle = (2.0 * np.pi) * ub
    return r * np.where((f % 2 == 1)[None, :], np.sin(angle), np.cos(angle))


def _check_generation(g):
    if not 0 <= int(g) < MAX_GENERATIONS:
        raise ValueError(f'generation {g}: the counter holds 0 <= g < 2^32')
    return int(g)


# ------------------------------------------------------------------------------ one generation
def gamma_host(fgamma, nfree):
    return fgamma * 2.38 / np.sqrt(2.0 * nfree)


def propose_host(theta, z, M, pstep, g, seed, fgamma=1.0, fepsilon=0.0, p_snooker=0.1,
                 details=False):
    """theta[nw, nfree], the history z[., nfree] whose first M >= 3 rows exist, pstep[nfree] ->
    (prop[nw, nfree], log_jac[nw], kind[nw] int32: 0 parallel, 1 snooker).  Per chain w, from
    TAG_PROPOSE at generation g:
        block 0: r1 = idx(u, M), r2 = idx(u', M - 1), r2 += (r2 >= r1);   block 1: u_s,
        rz = idx(u', M);   block 2: u_g;   blocks 3 + f // 2: the normals n_f
        u_s >= p_snooker:  prop = (theta + gamma (Z[r1] - Z[r2])) + (fepsilon pstep) n,
                           gamma = fgamma 2.38 / sqrt(2 nfree), log_jac = 0
        otherwise:         d = theta - Z[rz], D2 = d.d,
                           prop = theta + ((1.2 + u_g) ((Z[r1] - Z[r2]).d / D2)) d,
                           log_jac = 0.5 (nfree - 1) (ln |prop - Z[rz]|^2 - ln D2);
                           D2 not > 0 or log_jac not finite: prop = theta, log_jac = 0.
    details: also a namespace of r1, r2, rz, u_s, u_g, normals."""
    theta = np.asarray(theta, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    pstep = np.asarray(pstep, dtype=np.float64)
    nw, nfree = theta.shape
    M = int(M)
    if M < 3 or M > z.shape[0]:
        raise ValueError(f'a history of {M} rows (of {z.shape[0]}): at least 3')
    g = _check_generation(g)
    chains = np.arange(nw)
    ua, ub = block_uniforms_host(seed, 0, chains, g, TAG_PROPOSE)
    r1 = index_host(ua, M)
    r2 = index_host(ub, M - 1)
    r2 = r2 + (r2 >= r1)
    u_s, ub = block_uniforms_host(seed, 1, chains, g, TAG_PROPOSE)
    rz = index_host(ub, M)
    u_g, _ = block_uniforms_host(seed, 2, chains, g, TAG_PROPOSE)
    normals = normals_host(seed, chains, g, nfree)
    kind = (u_s < p_snooker).astype(np.int32)

    diff = z[r1] - z[r2]
    parallel = (theta + gamma_host(fgamma, nfree) * diff) + (fepsilon * pstep)[None, :] * normals
    with np.errstate(all='ignore'):
        d = theta - z[rz]
        D2 = np.sum(d * d, axis=1)
        proj = np.sum(diff * d, axis=1)
        c = (1.2 + u_g) * (proj / D2)
        snooker = theta + c[:, None] * d
        N2 = np.sum((snooker - z[rz])**2, axis=1)
        log_jac = (0.5 * (nfree - 1)) * (np.log(N2) - np.log(D2))
        ok = (D2 > 0.0) & np.isfinite(log_jac)
    snooker = np.where(ok[:, None], snooker, theta)
    log_jac = np.where(ok, log_jac, 0.0)
    prop = np.where((kind == 1)[:, None], snooker, parallel)
    log_jac = np.where(kind == 1, log_jac, 0.0)
    if details:
        return prop, log_jac, kind, types.SimpleNamespace(r1=r1, r2=r2, rz=rz, u_s=u_s, u_g=u_g,
                                                          normals=normals)
    return prop, log_jac, kind


def new_state_host(theta0, logp0, z0, capacity, thin_z=10):
    """The state accept_host works on, at sample 0: theta, logp, the chain store (row 0 = the
    starting state, count 1), Welford's sums (empty), the history z[Mcap, nfree] with M = len(z0)
    rows, g = 0."""
    theta = np.array(theta0, dtype=np.float64)
    z0 = np.asarray(z0, dtype=np.float64)
    nw, nfree = theta.shape
    cap = int(capacity)
    if cap < 1:
        raise ValueError('capacity >= 1')
    M = z0.shape[0]
    Mcap = M + nw * (cap // int(thin_z))
    st = types.SimpleNamespace(
        theta=theta, logp=np.array(logp0, dtype=np.float64), cap=cap,
        rows=np.full((nw, cap, nfree), np.nan), row_logp=np.full((nw, cap), np.nan),
        row_gen=np.zeros((nw, cap), np.int32), counts=np.zeros((nw, cap), np.int64),
        nrows=np.ones(nw, np.int32), overflow=np.zeros(nw, np.int32),
        mean=np.zeros((nw, nfree)), m2=np.zeros((nw, nfree)), nstat=np.zeros(nw, np.int64),
        z=np.full((Mcap, nfree), np.nan), M=M, Mcap=Mcap, g=0)
    st.z[:M] = z0
    st.rows[:, 0] = theta
    st.row_logp[:, 0] = st.logp
    st.counts[:, 0] = 1
    return st


def accept_margin_host(logp, logp_prop, log_jac, g, seed):
    """ln u - ((logp_prop - logp) + log_jac) per chain, u the first uniform of block 0 of
    TAG_ACCEPT: the chain accepts iff this is negative (NaN: it rejects)."""
    g = _check_generation(g)
    u, _ = block_uniforms_host(seed, 0, np.arange(len(logp)), g, TAG_ACCEPT)
    with np.errstate(invalid='ignore'):
        return np.log(u) - ((np.asarray(logp_prop) - np.asarray(logp)) + np.asarray(log_jac))


def accept_host(st, prop, logp_prop, log_jac, g, seed, append=False):
    """The rest of a generation on the state st (new_state_host), in place -> accepted[nw] int32.
    Chain w accepts iff ln u < (logp_prop - logp) + log_jac (a NaN on either side rejects, and so
    does a proposal at -inf).  Accept: theta, logp overwritten, a new row of the store opened
    (row_gen = g, count 1) -- or, without room, overflow set; reject: the last row's count
    raised.  A chain that has overflowed records nothing.  Then Welford's update with the state
    after the decision (nstat += 1, delta = x - mean, mean += delta / nstat, M2 += delta
    (x - mean)), and with append the states go to z[M : M + nw] (the caller raises M)."""
    g = _check_generation(g)
    prop = np.asarray(prop, dtype=np.float64)
    logp_prop = np.asarray(logp_prop, dtype=np.float64)
    log_jac = np.asarray(log_jac, dtype=np.float64)
    nw = st.theta.shape[0]
    u, _ = block_uniforms_host(seed, 0, np.arange(nw), g, TAG_ACCEPT)
    with np.errstate(invalid='ignore'):
        acc = np.log(u) < (logp_prop - st.logp) + log_jac
    if append and st.M + nw > st.Mcap:
        raise ValueError(f'appending {nw} rows to a history of {st.M}: its capacity is {st.Mcap}')
    st.theta[acc] = prop[acc]
    st.logp[acc] = logp_prop[acc]
    x = st.theta
    st.nstat += 1
    delta = x - st.mean
    st.mean += delta / st.nstat[:, None].astype(np.float64)
    st.m2 += delta * (x - st.mean)
    if append:
        st.z[st.M:st.M + nw] = x
    recording = (st.overflow == 0) & (st.nrows >= 1) & (st.nrows <= st.cap)
    new_row = recording & acc & (st.nrows < st.cap)
    w = np.where(new_row)[0]
    k = st.nrows[w]
    st.rows[w, k] = x[w]
    st.row_logp[w, k] = st.logp[w]
    st.row_gen[w, k] = g
    st.counts[w, k] = 1
    st.nrows[w] += 1
    st.overflow[recording & acc & ~new_row] = 1
    w = np.where(recording & ~acc)[0]
    st.counts[w, st.nrows[w] - 1] += 1
    return acc.astype(np.int32)


def gelman_rubin_host(mean, m2, n):
    """rhat[nfree] of nw chains of n states from their Welford sums mean[nw, nfree], m2[nw, nfree]:
    W = the mean over chains of M2 / (n - 1), B / n = the ddof = 1 variance of the chain means,
    R = sqrt(((n - 1) / n W + B / n) / W); NaN where W == 0, n < 2 or nw < 2."""
    mean, m2 = np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    nw, nfree = mean.shape
    n = int(n)
    if n < 2 or nw < 2:
        return np.full(nfree, np.nan)
    W = np.sum(m2 / (n - 1), axis=0) / nw
    grand = np.sum(mean, axis=0) / nw
    b_over_n = np.sum((mean - grand)**2, axis=0) / (nw - 1)
    with np.errstate(all='ignore'):
        return np.where(W == 0.0, np.nan, np.sqrt((((n - 1) / n) * W + b_over_n) / W))


def burn_cut(burn):
    """The first sample unique(burn) keeps: burn = 0 keeps everything, the starting state
    (sample 0) included; burn > 0 trims the first `burn` generations and the starting state they
    began from: samples burn + 1 onwards."""
    burn = int(burn)
    if burn < 0:
        raise ValueError('burn >= 0')
    return burn + 1 if burn > 0 else 0


def unique_host(st, burn=0):
    """(theta[n, nfree], counts[n] int64) of the state's chain store: the rows of all chains,
    chain by chain, their counts trimmed by row_gen to the samples from burn_cut(burn) on; rows
    left with nothing are dropped."""
    if np.any(st.overflow != 0):
        raise ValueError(f'chains {list(np.where(st.overflow != 0)[0])} overflowed their store')
    cut = burn_cut(burn)
    valid = np.arange(st.cap)[None, :] < st.nrows[:, None]
    begin = st.row_gen.astype(np.int64)
    kept = np.where(valid, np.maximum(begin + st.counts - np.maximum(begin, cut), 0), 0)
    keep = kept > 0
    return st.rows[keep], kept[keep]


def expand_host(rows, counts, nrows):
    """The dense chains [nw][nsamples, nfree] of a chain store."""
    return [np.repeat(rows[w, :nrows[w]], counts[w, :nrows[w]], axis=0)
            for w in range(rows.shape[0])]


def _refuse_start(logp):
    bad = np.where(~np.isfinite(logp))[0]
    if len(bad):
        raise ValueError(f'the starting states of chains {[int(w) for w in bad]} have no finite '
                         f'log-posterior ({[float(v) for v in logp[bad]]})')


def run_host(log_post, theta0, z0, ngen, seed=0, pstep=None, fgamma=1.0, fepsilon=0.0,
             p_snooker=0.1, thin_z=10, capacity=None, state=None):
    """The whole loop in NumPy.  log_post: theta[nw, nfree] -> [nw].  A first call (state=None)
    scores theta0 (starting states without a finite log-posterior: ValueError), lays out the
    store (capacity rows per chain, default ngen + 1) and the history (z0, at least 3 rows) and
    runs ngen generations; a call with state= (theta0, z0 ignored) continues with ngen more, and
    leaves the bits one long call leaves.  -> the state (new_state_host), with .chain (a list of
    the samples [nw, nfree], the starting states first), .accepted and .margin (lists of [nw] per
    generation: the decisions and accept_margin_host)."""
    st = state
    if st is None:
        theta0 = np.array(theta0, dtype=np.float64)
        logp0 = np.asarray(log_post(theta0), dtype=np.float64)
        _refuse_start(logp0)
        st = new_state_host(theta0, logp0, z0, ngen + 1 if capacity is None else capacity, thin_z)
        if st.M < 3:
            raise ValueError(f'a history of {st.M} rows: at least 3')
        st.pstep = np.ones(theta0.shape[1]) if pstep is None else np.asarray(pstep, float)
        st.chain, st.accepted, st.margin = [st.theta.copy()], [], []
    nw = st.theta.shape[0]
    for _ in range(int(ngen)):
        g = st.g + 1
        prop, log_jac, _ = propose_host(st.theta, st.z, st.M, st.pstep, g, seed, fgamma, fepsilon,
                                        p_snooker)
        logp_prop = np.asarray(log_post(prop), dtype=np.float64)
        append = g % thin_z == 0 and st.M + nw <= st.Mcap
        st.margin.append(accept_margin_host(st.logp, logp_prop, log_jac, g, seed))
        st.accepted.append(accept_host(st, prop, logp_prop, log_jac, g, seed, append))
        if append:
            st.M += nw
        st.g = g
        st.chain.append(st.theta.copy())
    return st


# ------------------------------------------------------------------------------ the device loop
class DEMC:
    """DEMC(log_post, nfree, pstep, seed=0, fgamma=1.0, fepsilon=0.0, p_snooker=0.1, thin_z=10):
    run_host on the device.  log_post: any callable from a float64 device tensor [nw, nfree] to
    [nw] (Retrieval.log_posterior, or torch arithmetic).

    start(theta0, z0, capacity) scores the starting states once; states without a finite
    log-posterior are refused with a ValueError that names the chains -- the only read-back.
    run(ngen): ngen generations, launches only; run(a) then run(b) leaves the bits of run(a + b).
    After a run: rhat() [nfree], acceptance() [nw], unique(burn) -> (theta[n, nfree],
    counts[n] int64), the form posterior_summary takes."""

    def __init__(self, log_post, nfree, pstep, seed=0, fgamma=1.0, fepsilon=0.0, p_snooker=0.1,
                 thin_z=10):
        from ._device import dev
        self.log_post = log_post
        self.nfree = int(nfree)
        pstep = np.asarray(pstep, dtype=np.float64)
        if pstep.shape != (self.nfree,):
            raise ValueError(f'pstep must have shape ({self.nfree},), got {pstep.shape}')
        if int(thin_z) < 1:
            raise ValueError('thin_z >= 1')
        self.pstep = dev(pstep)
        self.seed = int(seed) % 2**64
        self.fgamma, self.fepsilon = float(fgamma), float(fepsilon)
        self.p_snooker, self.thin_z = float(p_snooker), int(thin_z)
        self.g = None

    def _score(self, theta):
        import torch
        logp = self.log_post(theta)
        if not isinstance(logp, torch.Tensor) or not logp.is_cuda or \
                logp.dtype != torch.float64 or tuple(logp.shape) != (theta.shape[0],):
            raise ValueError(f'log_post must return a float64 device tensor of shape '
                             f'({theta.shape[0]},), got {type(logp).__name__} '
                             f'{getattr(logp, "dtype", "")} {tuple(getattr(logp, "shape", ()))}')
        return logp.contiguous()

    def start(self, theta0, z0, capacity):
        """theta0[nw, nfree]: the starting states; z0[M0 >= 3, nfree]: the initial history;
        capacity: the rows per chain of the store (ngen + 1 can never overflow)."""
        import torch
        from ._device import dev, require_gpu
        require_gpu()
        theta = dev(theta0).clone()
        z0 = dev(z0)
        if theta.dim() != 2 or theta.shape[1] != self.nfree or z0.dim() != 2 or \
                z0.shape[1] != self.nfree:
            raise ValueError(f'theta0 and z0 must have shape (., {self.nfree}), got '
                             f'{tuple(theta.shape)} and {tuple(z0.shape)}')
        nw, M0, cap = theta.shape[0], z0.shape[0], int(capacity)
        if nw < 1 or M0 < 3 or cap < 1:
            raise ValueError(f'{nw} chains, a history of {M0} rows, {cap} rows per chain: at '
                             'least 1, 3 and 1')
        logp = self._score(theta).clone()
        _refuse_start(logp.cpu().numpy())
        f64 = dict(dtype=torch.float64, device=theta.device)
        i32 = dict(dtype=torch.int32, device=theta.device)
        i64 = dict(dtype=torch.int64, device=theta.device)
        self.nw, self.cap = nw, cap
        self.theta, self.logp = theta, logp
        self.M, self.Mcap = M0, M0 + nw * (cap // self.thin_z)
        self.z = torch.empty((self.Mcap, self.nfree), **f64)
        self.z[:M0] = z0
        self.rows = torch.empty((nw, cap, self.nfree), **f64)
        self.row_logp = torch.empty((nw, cap), **f64)
        self.row_gen = torch.zeros((nw, cap), **i32)
        self.counts = torch.zeros((nw, cap), **i64)
        self.rows[:, 0] = theta
        self.row_logp[:, 0] = logp
        self.counts[:, 0] = 1
        self.nrows = torch.ones(nw, **i32)
        self.overflow = torch.zeros(nw, **i32)
        self.mean = torch.zeros((nw, self.nfree), **f64)
        self.m2 = torch.zeros((nw, self.nfree), **f64)
        self.nstat = torch.zeros(nw, **i64)
        self.prop = torch.empty((nw, self.nfree), **f64)
        self.log_jac = torch.empty(nw, **f64)
        self.kind = torch.empty(nw, **i32)
        self.accepted = torch.empty(nw, **i32)
        self.g = 0
        return self

    def _started(self):
        if self.g is None:
            raise ValueError('DEMC: start(theta0, z0, capacity) comes first')

    def run(self, ngen):
        """ngen more generations: two launches and one log_post call each, nothing read back."""
        from ._capi import call
        from ._device import _ptr, _stream
        self._started()
        if self.g + int(ngen) >= min(MAX_GENERATIONS, 2**31):
            raise ValueError(f'{self.g + int(ngen)} generations: row_gen holds fewer than 2^31')
        for _ in range(int(ngen)):
            g = self.g + 1
            call('pb_demc_propose', _ptr(self.prop), _ptr(self.log_jac), _ptr(self.kind),
                 _ptr(self.theta), _ptr(self.z), _ptr(self.pstep), g, self.seed, self.M,
                 self.fgamma, self.fepsilon, self.p_snooker, self.nfree, self.nw, _stream())
            logp_prop = self._score(self.prop)
            append = g % self.thin_z == 0 and self.M + self.nw <= self.Mcap
            call('pb_demc_accept', _ptr(self.theta), _ptr(self.logp), _ptr(self.prop),
                 _ptr(logp_prop), _ptr(self.log_jac), _ptr(self.rows), _ptr(self.row_logp),
                 _ptr(self.row_gen), _ptr(self.counts), _ptr(self.nrows), _ptr(self.overflow),
                 _ptr(self.mean), _ptr(self.m2), _ptr(self.nstat), _ptr(self.z),
                 _ptr(self.accepted), g, self.seed, self.M, self.Mcap, int(append), self.cap,
                 self.nfree, self.nw, _stream())
            if append:
                self.M += self.nw
            self.g = g
        return self

    def rhat(self):
        """[nfree]: Gelman & Rubin's R of the states after generations 1 .. g (pb_gelman_rubin)."""
        import torch
        from ._capi import call
        from ._device import _ptr, _stream
        self._started()
        out = torch.empty(self.nfree, dtype=torch.float64, device=self.theta.device)
        call('pb_gelman_rubin', _ptr(out), _ptr(self.mean), _ptr(self.m2), self.g, self.nfree,
             self.nw, _stream())
        return out

    def acceptance(self):
        """[nw]: the accepted fraction of the generations so far (the rows opened after the
        first); NaN for a chain that overflowed its store, and before the first generation."""
        import torch
        self._started()
        # (a tensor divisor: torch multiplies by the reciprocal of a Python scalar)
        rows = (self.nrows - 1).to(torch.float64)
        rate = rows / torch.full_like(rows, float(self.g)) if self.g else \
            torch.full_like(rows, float('nan'))
        return torch.where(self.overflow != 0, torch.full_like(rate, float('nan')), rate)

    def unique(self, burn=0):
        """(theta[n, nfree], counts[n] int64): unique_host on the device's store, with ordinary
        torch indexing (once per chain, not per generation).  A chain that overflowed its store:
        ValueError."""
        import torch
        self._started()
        over = torch.nonzero(self.overflow).reshape(-1).cpu().numpy()
        if len(over):
            raise ValueError(f'chains {[int(w) for w in over]} overflowed their store of '
                             f'{self.cap} rows: start() with a larger capacity')
        cut = burn_cut(burn)
        valid = torch.arange(self.cap, device=self.theta.device)[None, :] < self.nrows[:, None]
        begin = self.row_gen.to(torch.int64)
        kept = (begin + self.counts - torch.clamp(begin, min=cut)).clamp(min=0)
        kept = torch.where(valid, kept, torch.zeros_like(kept))
        keep = kept > 0
        return self.rows[keep].contiguous(), kept[keep].contiguous()
