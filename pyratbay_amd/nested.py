"""Nested sampling for the batched retrieval loop (Skilling 2006, Bayesian Anal. 1, 833): the
Bayesian evidence ln Z, its uncertainty, and the weighted dead points as unique rows plus int64
multiplicities, the form posterior_summary takes.  The reference hands its log-likelihood and a
prior transform to MultiNest (`sampler = multinest`, `nlive`) and makes an equal-weight posterior
of the output with weighted_to_equal; no parity with MultiNest's random stream or its ellipsoidal
rejection scheme is claimed.  The NumPy statements here (select_host, start_host, propose_host,
accept_host, finish_host, resample_host, run_host) ARE the specification: the kernels of
csrc/pb_nested.hip are tested against them, and they are tested on a target whose evidence is
known in closed form.

The sampler works in the unit cube on nlive live points.  One iteration `it` (from 1) removes the
K = batch lowest live points at once and replaces them by K walkers, so that one walk step is one
log-likelihood call over K points:

    select   rank the live points by logl ascending (ties to the lower index, NaN the lowest);
             the K lowest die in that order.  Dead point j, with n = nlive - j:
                 ln w = (logl + ln X) + ln(-expm1(-1 / n))   (-inf for a NaN logl)
                 ln X -= 1 / n;   ln Z = logaddexp(ln Z, ln w)
             Lstar = logl of the last of them; remain = logaddexp(ln Z, Ltop + ln X) - ln Z with
             Ltop the logl of the highest survivor: the stopping quantity.
    start    slot k begins at survivor idx(u, nsurv), u the first uniform of block 0 at
             (0, k, it, TAG_NESTED_START).
    walk     nsteps differential-evolution steps constrained to logl > Lstar; step s of iteration
             it is the global step q = (it - 1) nsteps + s < 2^32, drawn at (block, k, q,
             TAG_NESTED_STEP): block 0: a = idx(u, nsurv), b = idx(u', nsurv - 1), b += (b >= a);
             block 1: gamma = 1 if u_m < p_unit else fgamma 2.38 / sqrt(2 nfree);
                 prop = cur + gamma (U[surv a] - U[surv b]),   inside = all(0 < prop < 1)
             A slot outside the cube is evaluated at cur instead, and can not accept.  Accept iff
             inside and logl_prop > Lstar (strict; a NaN rejects).  After the last step slot k
             takes the place of dead point k in the live set.  A slot without a single accept in
             an iteration duplicates a survivor: it is counted in `stuck`, never hidden.
    finish   (at any time, without disturbing the run) the live points join with
             ln w = (logl + ln X) - ln(nlive) in index order; ln Z, the information
             H = sum p ln L - ln Z with p = exp(ln w - ln Z), ln Z_err = sqrt(H / nlive), and the
             normalised cdf of p, summed in chunks (finish_host states the order).
    resample the reference's weighted_to_equal as a histogram: nsamples uniforms at
             TAG_NESTED_RESAMPLE, index = the first i with cdf[i] > u.

idx, the uniforms and Philox's addressing are those of sampler.py and csrc/pb_philox.h.
"""
import types

import numpy as np

from ._capi import constant
from .sampler import (MAX_GENERATIONS, block_uniforms_host, gamma_host, index_host,
                      uniforms_host)

TAG_NESTED_START, TAG_NESTED_STEP, TAG_NESTED_RESAMPLE = 3, 4, 5
MAX_LIVE = constant('PB_NESTED_MAX_LIVE')
MAX_PARAMS = constant('PB_RETRIEVAL_MAX_PARAMS')
FINISH_CHUNKS = 256                 # the chunks finish sums in: one per thread of its block
MAX_RESAMPLE = 2**32


def _check_counter(what, v):
    if not 0 <= int(v) < MAX_GENERATIONS:
        raise ValueError(f'{what} {v}: the counter holds 0 <= {what} < 2^32')
    return int(v)


def _check_batch(K, nlive):
    K, nlive = int(K), int(nlive)
    if nlive > MAX_LIVE:
        raise ValueError(f'{nlive} live points: at most {MAX_LIVE}')
    if not 1 <= K <= nlive - 2:
        raise ValueError(f'a batch of {K} with {nlive} live points: 1 <= batch <= nlive - 2')
    return K, nlive


# ------------------------------------------------------------------------------ one iteration
def rank_host(logl):
    """The live points' indices by logl ascending; ties go to the lower index, NaN ranks as the
    lowest (below -inf)."""
    logl = np.asarray(logl, dtype=np.float64)
    nan = np.isnan(logl)
    return np.lexsort((np.arange(len(logl)), np.where(nan, -np.inf, logl), ~nan))


def select_host(live_logl, ln_x, ln_z, K):
    """live_logl[nlive], ln X and ln Z before -> a namespace of dead_idx[K], surv_idx[nlive - K]
    (rank order), dead_logl[K], dead_logw[K], ln_x, ln_z after, lstar and remain (module
    docstring: select)."""
    logl = np.asarray(live_logl, dtype=np.float64)
    K, nlive = _check_batch(K, len(logl))
    order = rank_host(logl)
    dead_idx, surv_idx = order[:K], order[K:]
    dead_logl = logl[dead_idx]
    dead_logw = np.empty(K)
    ln_x, ln_z = float(ln_x), float(ln_z)
    with np.errstate(invalid='ignore'):
        for j in range(K):
            inv = 1.0 / float(nlive - j)
            shell = np.log(-np.expm1(-inv))
            lw = -np.inf if np.isnan(dead_logl[j]) else (dead_logl[j] + ln_x) + shell
            dead_logw[j] = lw
            ln_x = ln_x - inv
            ln_z = float(np.logaddexp(ln_z, lw))
        top = logl[surv_idx[-1]]
        remain = float(np.logaddexp(ln_z, top + ln_x) - ln_z)
    return types.SimpleNamespace(dead_idx=dead_idx, surv_idx=surv_idx, dead_logl=dead_logl,
                                 dead_logw=dead_logw, ln_x=ln_x, ln_z=ln_z,
                                 lstar=float(dead_logl[-1]), remain=remain)


def start_host(live_u, live_logl, surv_idx, K, it, seed):
    """-> (cur[K, nfree], cur_logl[K], pick[K]): slot k starts at live point pick[k] =
    surv_idx[idx(u, nsurv)], u the first uniform of block 0 at (0, k, it, TAG_NESTED_START)."""
    it = _check_counter('it', it)
    surv_idx = np.asarray(surv_idx)
    u, _ = block_uniforms_host(seed, 0, np.arange(int(K)), it, TAG_NESTED_START)
    pick = surv_idx[index_host(u, len(surv_idx))]
    return np.array(live_u[pick], dtype=np.float64), np.array(live_logl[pick], np.float64), pick


def propose_host(cur, live_u, surv_idx, q, seed, fgamma=1.0, p_unit=0.1, details=False):
    """cur[K, nfree], the live cube, the survivors -> (point[K, nfree], inside[K] int32): the
    proposal of global step q (module docstring: walk) where it lies inside the cube, cur where
    it does not.  details: also a namespace of a, b (indices into surv_idx), gamma and prop."""
    q = _check_counter('q', q)
    cur = np.asarray(cur, dtype=np.float64)
    live_u = np.asarray(live_u, dtype=np.float64)
    surv_idx = np.asarray(surv_idx)
    K, nfree = cur.shape
    nsurv = len(surv_idx)
    if nsurv < 2:
        raise ValueError(f'{nsurv} survivors: at least 2')
    slots = np.arange(K)
    ua, ub = block_uniforms_host(seed, 0, slots, q, TAG_NESTED_STEP)
    a = index_host(ua, nsurv)
    b = index_host(ub, nsurv - 1)
    b = b + (b >= a)
    um, _ = block_uniforms_host(seed, 1, slots, q, TAG_NESTED_STEP)
    gamma = np.where(um < p_unit, 1.0, gamma_host(fgamma, nfree))
    prop = cur + gamma[:, None] * (live_u[surv_idx[a]] - live_u[surv_idx[b]])
    with np.errstate(invalid='ignore'):
        inside = np.all((prop > 0.0) & (prop < 1.0), axis=1)
    point = np.where(inside[:, None], prop, cur)
    inside = inside.astype(np.int32)
    if details:
        return point, inside, types.SimpleNamespace(a=a, b=b, gamma=gamma, prop=prop)
    return point, inside


def new_state_host(live_u, live_logl, K):
    """The state of a run before its first iteration."""
    live_u = np.array(live_u, dtype=np.float64)
    nlive, nfree = live_u.shape
    K, nlive = _check_batch(K, nlive)
    return types.SimpleNamespace(
        live_u=live_u, live_logl=np.array(live_logl, dtype=np.float64), K=K,
        ln_x=0.0, ln_z=-np.inf, lstar=np.nan, remain=np.inf, it=0,
        cur=np.full((K, nfree), np.nan), cur_logl=np.full(K, np.nan),
        naccept=np.zeros(K, np.int64), acc_it=np.zeros(K, np.int32), stuck=np.zeros(K, np.int64),
        dead_u=np.empty((0, nfree)), dead_logl=np.empty(0), dead_logw=np.empty(0))


def accept_host(st, point, logl_prop, inside, lstar, dead_idx=None):
    """The rest of a walk step on the state st, in place -> accepted[K] int32.  Slot k accepts iff
    inside[k] and logl_prop[k] > lstar: cur and cur_logl overwritten, naccept and acc_it (the
    accepts of this iteration) raised.  dead_idx (the last step of an iteration): then
    live[dead_idx[k]] = cur[k], and stuck[k] += 1 where acc_it[k] == 0."""
    point = np.asarray(point, dtype=np.float64)
    logl_prop = np.asarray(logl_prop, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        acc = (np.asarray(inside) != 0) & (logl_prop > lstar)
    st.cur[acc] = point[acc]
    st.cur_logl[acc] = logl_prop[acc]
    st.naccept += acc
    st.acc_it += acc
    if dead_idx is not None:
        st.live_u[dead_idx] = st.cur
        st.live_logl[dead_idx] = st.cur_logl
        st.stuck += st.acc_it == 0
    return acc.astype(np.int32)


# ------------------------------------------------------------------------------ the result
def _chunked_cumsum(x, chunks=FINISH_CHUNKS):
    """(the running sum of x, its total), in finish's order: `chunks` chunks of
    ceil(n / chunks) consecutive elements; every chunk is summed from 0 in index order, the chunk
    sums are summed in chunk order, and the running sum within a chunk starts from the sum of
    the chunks before it."""
    n = len(x)
    per = max(-(-n // chunks), 1)
    padded = np.zeros(chunks * per)
    padded[:n] = x
    padded = padded.reshape(chunks, per)
    sums = np.cumsum(padded, axis=1)[:, -1]
    before = np.concatenate(([0.0], np.cumsum(sums)[:-1]))
    running = np.cumsum(np.concatenate((before[:, None], padded), axis=1), axis=1)[:, 1:]
    return running.reshape(-1)[:n], float(np.cumsum(sums)[-1])


def finish_host(dead_logl, dead_logw, live_logl, ln_x):
    """The dead store, the live points and ln X -> a namespace of logl[n], logw[n] (the dead
    points, then the live ones at ln w = (logl + ln X) - ln(nlive); -inf for a NaN logl), ln_z,
    info (H), ln_z_err and cdf[n].  With m = max ln w and e = exp(ln w - m) (0 where ln w is
    -inf): S = sum e, ln Z = m + ln S, H = (sum e ln L over e > 0) / S - ln Z,
    ln Z_err = sqrt(max(H, 0) / nlive), cdf = running sum of e / S; sums as _chunked_cumsum."""
    live_logl = np.asarray(live_logl, dtype=np.float64)
    nlive = len(live_logl)
    with np.errstate(all='ignore'):
        live_logw = np.where(np.isnan(live_logl), -np.inf,
                             (live_logl + ln_x) - np.log(float(nlive)))
        logl = np.concatenate((np.asarray(dead_logl, dtype=np.float64), live_logl))
        logw = np.concatenate((np.asarray(dead_logw, dtype=np.float64), live_logw))
        m = np.fmax.reduce(logw, initial=-np.inf)
        e = np.where(logw == -np.inf, 0.0, np.exp(logw - m))
        running, S = _chunked_cumsum(e)
        _, hsum = _chunked_cumsum(np.where(e > 0.0, e * logl, 0.0))
        ln_z = m + np.log(S)
        info = hsum / S - ln_z
        ln_z_err = np.sqrt(np.fmax(info, 0.0) / nlive)
        cdf = running / S
    return types.SimpleNamespace(logl=logl, logw=logw, ln_z=float(ln_z), info=float(info),
                                 ln_z_err=float(ln_z_err), cdf=cdf)


def resample_uniforms_host(seed, nsamples):
    """[nsamples]: sample s is the uniform s % 2 of block 0 at (0, s // 2, 0,
    TAG_NESTED_RESAMPLE)."""
    nsamples = int(nsamples)
    if not 0 <= nsamples <= MAX_RESAMPLE:
        raise ValueError(f'{nsamples} samples: at most 2^32')
    s = np.arange(nsamples)
    ua, ub = block_uniforms_host(seed, 0, s // 2, 0, TAG_NESTED_RESAMPLE)
    return np.where(s % 2 == 0, ua, ub)


def resample_host(cdf, nsamples, seed):
    """counts[n] int64: how many of nsamples uniforms fall on each row, index = the first i with
    cdf[i] > u, clipped to the last row (the reference's weighted_to_equal as a histogram)."""
    cdf = np.asarray(cdf, dtype=np.float64)
    u = resample_uniforms_host(seed, nsamples)
    index = np.minimum(np.searchsorted(cdf, u, side='right'), len(cdf) - 1)
    return np.bincount(index, minlength=len(cdf)).astype(np.int64)


def default_batch(nlive):
    return max(1, min(int(nlive) // 4, int(nlive) - 2))


def default_nsteps(nfree):
    return max(20, 5 * int(nfree))


def run_host(log_like, prior_transform, nlive, batch, nsteps, niter, seed=0, nfree=None,
             fgamma=1.0, p_unit=0.1, dlogz=None, check_every=1, state=None):
    """The whole loop in NumPy.  log_like: theta[n, nfree] -> [n]; prior_transform: cube[n, nfree]
    -> theta.  A first call (state=None, nfree required) draws the live cube
    uniforms_host(seed, nlive, nfree), scores it and runs niter iterations; with dlogz it stops
    after the first iteration, of every check_every-th, that leaves remain < dlogz (niter is then
    the most it runs).  A call with state= continues and leaves the bits one long call leaves.
    -> the state (new_state_host), with .dead_idx and .accepted (lists per iteration: [K] and
    [nsteps, K]) and .margin (logl_prop - Lstar, [nsteps, K] per iteration)."""
    st = state
    if st is None:
        cube = uniforms_host(seed, int(nlive), int(nfree))
        logl = np.asarray(log_like(prior_transform(cube)), dtype=np.float64)
        st = new_state_host(cube, logl, batch)
        st.dead_idx, st.accepted, st.margin = [], [], []
    K, nsteps = st.K, int(nsteps)
    if nsteps < 1:
        raise ValueError('nsteps >= 1')
    for _ in range(int(niter)):
        it = _check_counter('it', st.it + 1)
        _check_counter('q', it * nsteps - 1)
        sel = select_host(st.live_logl, st.ln_x, st.ln_z, K)
        st.ln_x, st.ln_z, st.lstar, st.remain = sel.ln_x, sel.ln_z, sel.lstar, sel.remain
        st.dead_u = np.concatenate((st.dead_u, st.live_u[sel.dead_idx]))
        st.dead_logl = np.concatenate((st.dead_logl, sel.dead_logl))
        st.dead_logw = np.concatenate((st.dead_logw, sel.dead_logw))
        st.cur, st.cur_logl, _ = start_host(st.live_u, st.live_logl, sel.surv_idx, K, it, seed)
        st.acc_it[:] = 0
        accepted, margin = [], []
        for s in range(nsteps):
            q = (it - 1) * nsteps + s
            point, inside = propose_host(st.cur, st.live_u, sel.surv_idx, q, seed, fgamma, p_unit)
            logl = np.asarray(log_like(prior_transform(point)), dtype=np.float64)
            with np.errstate(invalid='ignore'):
                margin.append(logl - st.lstar)
            accepted.append(accept_host(st, point, logl, inside, st.lstar,
                                        sel.dead_idx if s == nsteps - 1 else None))
        st.dead_idx.append(sel.dead_idx)
        st.accepted.append(np.array(accepted))
        st.margin.append(np.array(margin))
        st.it = it
        if dlogz is not None and it % int(check_every) == 0 and st.remain < dlogz:
            break
    return st


# ------------------------------------------------------------------------------ the device loop
class NestedSampler:
    """NestedSampler(log_like, prior_transform, nfree, nlive, batch=None, nsteps=None, seed=0,
    fgamma=1.0, p_unit=0.1): run_host on the device.  log_like: any callable from a float64
    device tensor theta[n, nfree] to [n] (Retrieval.log_likelihood, or torch arithmetic);
    prior_transform: cube[n, nfree] -> theta (Retrieval.prior_transform).

    start() draws and scores the live points.  run(niter): launches only, nothing read back;
    run(a) then run(b) leaves the bits of run(a + b).  run_until(dlogz, check_every, max_iter)
    reads back one double, `remain`, per check.  Then logz() -> (ln Z, ln Z_err, H) as a device
    tensor, weighted() -> (theta, ln w, ln L), unique() -> (theta[n, nfree], counts[n] int64),
    efficiency() and stuck().  The run does not cluster: modes() separates the posterior's modes
    afterwards (modes.py), and unique(mode=m) is the posterior of one of them.

    The defaults batch = nlive // 4 and nsteps = max(20, 5 nfree) come from the Gaussian target
    of the tests (a batch of nlive / 2 biased ln Z by about -0.07 there); they are unmeasured on
    a real retrieval.  A walk that is too short shows as a high stuck() and a low efficiency()."""

    def __init__(self, log_like, prior_transform, nfree, nlive, batch=None, nsteps=None, seed=0,
                 fgamma=1.0, p_unit=0.1):
        self.log_like, self.prior_transform = log_like, prior_transform
        self.nfree, self.nlive = int(nfree), int(nlive)
        if not 1 <= self.nfree <= MAX_PARAMS:
            raise ValueError(f'{self.nfree} free parameters: 1 to {MAX_PARAMS}')
        self.K, _ = _check_batch(default_batch(nlive) if batch is None else batch, nlive)
        self.nsteps = default_nsteps(nfree) if nsteps is None else int(nsteps)
        if self.nsteps < 1:
            raise ValueError('nsteps >= 1')
        self.seed = int(seed) % 2**64
        self.fgamma, self.p_unit = float(fgamma), float(p_unit)
        self.it = None
        self.trace = None           # a list: run() appends (dead_idx[K], accepted[nsteps, K])

    def _score(self, cube):
        import torch
        logl = self.log_like(self.prior_transform(cube))
        if not isinstance(logl, torch.Tensor) or not logl.is_cuda or \
                logl.dtype != torch.float64 or tuple(logl.shape) != (cube.shape[0],):
            raise ValueError(f'log_like must return a float64 device tensor of shape '
                             f'({cube.shape[0]},), got {type(logl).__name__} '
                             f'{getattr(logl, "dtype", "")} {tuple(getattr(logl, "shape", ()))}')
        return logl.contiguous()

    def start(self):
        import torch
        from ._capi import call
        from ._device import _ptr, _stream, require_gpu
        require_gpu()
        f64 = dict(dtype=torch.float64, device='cuda')
        i32 = dict(dtype=torch.int32, device='cuda')
        i64 = dict(dtype=torch.int64, device='cuda')
        K, nfree, nlive = self.K, self.nfree, self.nlive
        self.live_u = torch.empty((nlive, nfree), **f64)
        call('pb_philox_uniform', _ptr(self.live_u), self.seed, nlive, nfree, _stream())
        self.live_logl = self._score(self.live_u).clone()
        # ln X, ln Z, Lstar, remain
        self.state = torch.tensor([0.0, -np.inf, np.nan, np.inf], **f64)
        self.dead_idx = torch.zeros(K, **i32)
        self.surv_idx = torch.zeros(nlive - K, **i32)
        self.cur = torch.empty((K, nfree), **f64)
        self.cur_logl = torch.empty(K, **f64)
        self.point = torch.empty((K, nfree), **f64)
        self.inside = torch.empty(K, **i32)
        self.draw_a, self.draw_b = torch.empty(K, **i32), torch.empty(K, **i32)
        self.draw_gamma = torch.empty(K, **f64)
        self.accepted = torch.empty(K, **i32)
        self.naccept = torch.zeros(K, **i64)
        self.acc_it = torch.zeros(K, **i32)
        self.stuck_slots = torch.zeros(K, **i64)
        self.dead_cap = 0
        self._grow(16 * K)
        self.it = 0
        return self

    def _started(self):
        if self.it is None:
            raise ValueError('NestedSampler: start() comes first')

    @property
    def ndead(self):
        return self.it * self.K

    def _grow(self, rows):
        """The dead store with room for `rows` rows: doubled on the host's count, which needs no
        read-back (iteration it has written it K rows)."""
        import torch
        if rows <= self.dead_cap:
            return
        cap = max(self.dead_cap, 1)
        while cap < rows:
            cap *= 2
        old = (self.dead_u, self.dead_logl, self.dead_logw) if self.dead_cap else None
        f64 = dict(dtype=torch.float64, device='cuda')
        self.dead_u = torch.empty((cap, self.nfree), **f64)
        self.dead_logl = torch.empty(cap, **f64)
        self.dead_logw = torch.empty(cap, **f64)
        if old is not None:
            n = self.ndead
            for new, was in zip((self.dead_u, self.dead_logl, self.dead_logw), old):
                new[:n] = was[:n]
        self.dead_cap = cap

    def run(self, niter):
        """niter more iterations: one select, and per walk step one propose, one prior transform,
        one log-likelihood and one accept; nothing read back."""
        import torch
        from ._capi import call
        from ._device import _ptr, _stream
        self._started()
        K, nfree, nlive, nsteps = self.K, self.nfree, self.nlive, self.nsteps
        _check_counter('it', self.it + int(niter))
        _check_counter('q', max((self.it + int(niter)) * nsteps - 1, 0))
        for _ in range(int(niter)):
            it = self.it + 1
            self._grow(it * K)
            call('pb_nested_select', _ptr(self.dead_idx), _ptr(self.surv_idx), _ptr(self.dead_u),
                 _ptr(self.dead_logl), _ptr(self.dead_logw), _ptr(self.state), _ptr(self.live_u),
                 _ptr(self.live_logl), self.ndead, self.dead_cap, K, nlive, nfree, _stream())
            steps = []
            for s in range(nsteps):
                q = (it - 1) * nsteps + s
                call('pb_nested_propose', _ptr(self.point), _ptr(self.inside), _ptr(self.draw_a),
                     _ptr(self.draw_b), _ptr(self.draw_gamma), _ptr(self.cur),
                     _ptr(self.cur_logl), _ptr(self.acc_it), _ptr(self.live_u),
                     _ptr(self.live_logl), _ptr(self.surv_idx), it, q, self.seed, self.fgamma,
                     self.p_unit, int(s == 0), nlive, nfree, K, _stream())
                logl = self._score(self.point)
                call('pb_nested_accept', _ptr(self.cur), _ptr(self.cur_logl), _ptr(self.point),
                     _ptr(logl), _ptr(self.inside), _ptr(self.state), _ptr(self.naccept),
                     _ptr(self.acc_it), _ptr(self.stuck_slots), _ptr(self.accepted),
                     _ptr(self.live_u), _ptr(self.live_logl), _ptr(self.dead_idx),
                     int(s == nsteps - 1), nlive, nfree, K, _stream())
                if self.trace is not None:
                    steps.append(self.accepted.clone())
            if self.trace is not None:
                self.trace.append((self.dead_idx.clone(), torch.stack(steps)))
            self.it = it
        return self

    def run_until(self, dlogz=0.5, check_every=10, max_iter=100000):
        """Iterations until remain = logaddexp(ln Z, Ltop + ln X) - ln Z < dlogz, looked at after
        every check_every-th iteration (one double read back per look), max_iter at the most."""
        self._started()
        check_every = int(check_every)
        if check_every < 1:
            raise ValueError('check_every >= 1')
        done = 0
        while done < int(max_iter):
            step = min(check_every, int(max_iter) - done)
            self.run(step)
            done += step
            if step == check_every and self.state[3].item() < dlogz:
                break
        return self

    def _finish(self):
        import torch
        from ._capi import call
        from ._device import _ptr, _stream
        self._started()
        n = self.ndead + self.nlive
        f64 = dict(dtype=torch.float64, device='cuda')
        out = torch.empty(3, **f64)
        logw, logl, cdf = torch.empty(n, **f64), torch.empty(n, **f64), torch.empty(n, **f64)
        call('pb_nested_finish', _ptr(out), _ptr(logw), _ptr(logl), _ptr(cdf),
             _ptr(self.dead_logl), _ptr(self.dead_logw), _ptr(self.live_logl), _ptr(self.state),
             self.ndead, self.nlive, _stream())
        return out, logw, logl, cdf

    def _cube(self):
        import torch
        return torch.cat((self.dead_u[:self.ndead], self.live_u))

    def logz(self):
        """[3] on the device: ln Z, ln Z_err = sqrt(H / nlive), H."""
        return self._finish()[0]

    def weighted(self):
        """(theta[n, nfree], ln w[n], ln L[n]): the dead points in the order they died, then the
        live points; theta is the prior transform of the stored cube rows."""
        _, logw, logl, _ = self._finish()
        return self.prior_transform(self._cube()), logw, logl

    def _resample(self, cdf, nsamples):
        import torch
        from ._capi import call
        from ._device import _ptr, _stream
        n = cdf.shape[0]
        counts = torch.empty(n, dtype=torch.int64, device='cuda')
        call('pb_nested_resample', _ptr(counts), _ptr(cdf), n, int(nsamples), self.seed, _stream())
        return counts

    def modes(self, nsamples=4096, knn=10, link=1.0, min_mode=None, max_modes=16):
        """The posterior modes of the run so far (modes.modes_host on the device; it changes
        nothing of the run and keeps no state, so it can be taken at any time): a namespace of
        device tensors nmodes (an int), mode[n] int32 in weighted()'s order, ln_z[nmodes],
        info[nmodes] and fraction[nmodes] (the local evidences, their information and their
        shares of the evidence), rows (the rows the modes were found on), labels (theirs) and
        ell2 (the squared linking length in the unit cube).  Launches only, but for two counts
        read back once each: the number of rows and nmodes.  A local evidence has no error bar
        (modes.py says why; profiles/modes.md has the measured scatter)."""
        import torch
        from . import modes as md
        from ._capi import call
        from ._device import _ptr, _stream
        out, logw, logl, cdf = self._finish()
        cube = self._cube().contiguous()
        N, nfree = cube.shape
        md._check_link(2, nfree, knn, max_modes)
        min_mode = md.default_min_mode(nfree) if min_mode is None else int(min_mode)
        i32 = dict(dtype=torch.int32, device='cuda')
        f64 = dict(dtype=torch.float64, device='cuda')
        counts = self._resample(cdf, min(N, int(nsamples)))
        rows = torch.empty(MAX_LIVE, dtype=torch.int64, device='cuda')
        nrows = torch.empty(1, dtype=torch.int64, device='cuda')
        call('pb_modes_rows', _ptr(rows), _ptr(nrows), _ptr(counts), N, MAX_LIVE, _stream())
        n = int(nrows.item())
        if n > MAX_LIVE:
            raise ValueError(f'{n} rows: at most {MAX_LIVE} (nsamples = {nsamples})')
        rows = rows[:n]
        mode = torch.zeros(N, **i32)
        labels = torch.zeros(n, **i32)
        ell2 = torch.zeros(1, **f64)
        nmodes = 1
        if n >= 2:
            R = cube[rows].contiguous()
            count = torch.empty(1, **i32)
            dk = torch.empty(n, **f64)
            bits = torch.empty(n * ((n + 31) // 32), **i32)
            call('pb_modes_link', _ptr(labels), _ptr(count), _ptr(ell2), _ptr(dk), _ptr(bits),
                 _ptr(R), n, nfree, int(knn), float(link), min_mode, int(max_modes), _stream())
            call('pb_modes_assign', _ptr(mode), _ptr(cube), _ptr(R), _ptr(labels), N, n, nfree,
                 _stream())
            nmodes = int(count.item())
        ln_z, info, fraction = (torch.empty(nmodes, **f64) for _ in range(3))
        call('pb_modes_evidence', _ptr(ln_z), _ptr(info), _ptr(fraction), _ptr(logw), _ptr(logl),
             _ptr(mode), _ptr(out), N, nmodes, _stream())
        return types.SimpleNamespace(nmodes=nmodes, mode=mode, ln_z=ln_z, info=info,
                                     fraction=fraction, rows=rows, labels=labels, ell2=ell2[0])

    def unique(self, burn=0, nsamples=None, mode=None):
        """(theta[n, nfree], counts[n] int64): the equal-weight posterior as rows and
        multiplicities, nsamples draws (default: as many as there are rows, like the reference's
        weighted_to_equal); rows nothing fell on are dropped.  Nested sampling has no burn-in:
        burn != 0 is refused.  mode=m: only the rows modes() assigns to mode m, with the counts
        of the same one resample, so that the rows of the modes partition those of unique() and
        their counts add up; an m outside 0 .. nmodes - 1 is refused."""
        if int(burn) != 0:
            raise ValueError(f'burn = {burn}: nested sampling has no burn-in to trim')
        _, _, _, cdf = self._finish()
        n = cdf.shape[0]
        nsamples = n if nsamples is None else int(nsamples)
        counts = self._resample(cdf, nsamples)
        keep = counts > 0
        if mode is not None:
            found = self.modes()
            if int(mode) != mode or not 0 <= int(mode) < found.nmodes:
                raise ValueError(f'mode = {mode}: the run has the modes 0 to {found.nmodes - 1}')
            keep = keep & (found.mode == int(mode))
        theta = self.prior_transform(self._cube()[keep].contiguous())
        return theta, counts[keep].contiguous()

    def efficiency(self):
        """The accepted fraction of the walk steps so far (a device scalar; NaN before the first
        iteration)."""
        import torch
        self._started()
        total = self.naccept.sum().to(torch.float64)
        steps = float(self.it * self.nsteps * self.K)
        return total / torch.full_like(total, steps) if steps else \
            torch.full_like(total, float('nan'))

    def stuck(self):
        """How many replacements made not a single accepted step, and so duplicate a survivor
        (a device scalar, int64), out of it * batch."""
        self._started()
        return self.stuck_slots.sum()
