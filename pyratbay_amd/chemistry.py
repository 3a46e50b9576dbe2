"""Gas-phase thermochemical equilibrium per (walker, layer) cell: the VMRs that the reference
takes from chemcat (Atmosphere.calc_profiles, pyrat/atmosphere.py:445-473) for the parameters
[M/H], [X/H] and X/Y, solved by this package from the caller's table of G°/RT.

The caller supplies the thermochemistry like radiative_equilibrium(heat_capacity=...) takes cp/R:
ChemNetwork(species, elements, stoich, gibbs_temps, gibbs_over_RT, base_dex).  Someone with chemcat
exports that table once; nothing here reads chemcat.  The equilibrium of an ideal gas mixture is
the unique minimum of a convex function, so a converged solver gives chemcat's VMRs up to its own
convergence; no parity with chemcat's bits is claimed.

Two forms of the same arithmetic:
  * host forms in NumPy: ChemNetwork.element_abundances_host, equilibrium_host, hybrid_host;
  * equilibrium_vmr: temps[nw, L], params[nw, npar] -> vmr[nw, L, S], status[nw, L] on the device,
    one launch of pb_equilibrium_vmr (csrc/pb_chemistry.hip), nothing read back.

The solver is the reduced Newton iteration of Gordon & McBride (NASA RP-1311, 1994, section 2.3,
gas phase only) on ln n_i and ln n, from the same cold start in every cell:
    mu_i = g_i + ln n_i - ln n + ln p                                   (p in bar)
    rows k < E:  sum_j (sum_i a_ik a_ij n_i) pi_j + (sum_i a_ik n_i) dln n
                     = b_k - sum_i a_ik n_i + sum_i a_ik n_i mu_i
    last row:    sum_j (sum_i a_ij n_i) pi_j + (sum_i n_i - n) dln n = n - sum_i n_i + sum_i n_i mu_i
    dln n_i = -mu_i + dln n + sum_j a_ij pi_j
    lambda = min(1, l1, l2)                                              (RP-1311 eqs. 3.1-3.3)
The iterate is carried as ln n_i (n_i = exp(ln n_i) may underflow to 0 and then adds 0 to every
sum); the ratio in l2 is therefore read from the logarithms, -(ln n_i - ln n).

Out of scope: condensates, ions, networks above 64 species, re-equilibrating inside
radiative_equilibrium (profiles/chemistry.md).
"""
import ctypes as C

import numpy as np

from ._capi import constant, struct

MAX_NET_SPECIES, MAX_ELEMENTS, MAX_HYBRID = (constant('PB_CHEM_MAX_SPECIES'),
                                             constant('PB_CHEM_MAX_ELEMENTS'),
                                             constant('PB_CHEM_MAX_HYBRID'))
MAX_ITERATIONS = 200
# The largest full Newton step (on the major species and on ln n) at which a cell counts as
# converged.  Newton converges quadratically, so the error left after such a step is its square;
# what limits the step from below is the rounding of the residuals b_k - sum_i a_ik n_i, a few
# units of 1e-16 times the condition of the system.  1e-12 keeps two orders above that floor for
# exp and log that differ in their last bits (profiles/chemistry.md has the iteration counts).
TOLERANCE = 1.0e-12
# temperature <= 0 or NaN: a walker rejected before the chemistry
STATUS_REJECTED = constant('PB_CHEM_REJECTED')
STATUS_TEMPERATURE = constant('PB_CHEM_TEMPERATURE')        # temperature outside gibbs_temps
# an X/Y <= 0, or an elemental abundance that is not finite and > 0
STATUS_RATIO = constant('PB_CHEM_RATIO')
# MAX_ITERATIONS without a converged full step
STATUS_NOT_CONVERGED = constant('PB_CHEM_NOT_CONVERGED')
STATUS_NAMES = {STATUS_REJECTED: 'temperature <= 0',
                STATUS_TEMPERATURE: 'temperature outside the Gibbs table',
                STATUS_RATIO: 'an element ratio <= 0 or a non-finite abundance',
                STATUS_NOT_CONVERGED: 'not converged'}
_MINOR = 1.0e-8               # n_i / n at and below which a species is a minor one
_LN_MINOR = 9.2103404         # RP-1311 eq. 3.2: -ln(1e-4)


def _species_limit():
    from .atmosphere import MAX_SPECIES
    return min(MAX_NET_SPECIES, MAX_SPECIES)


def gauss_solve(A, r):
    """x of A x = r for stacks A[c, N, N], r[c, N]: Gaussian elimination with partial pivoting in
    the device's form -- the pivot row found by compare-and-swap down the column, so that no row is
    addressed by a computed index."""
    A, r = np.array(A, float), np.array(r, float)
    N = A.shape[1]
    with np.errstate(all='ignore'):
        for k in range(N):
            for i in range(k + 1, N):
                swap = np.abs(A[:, i, k]) > np.abs(A[:, k, k])
                row_i, row_k = A[:, i, :].copy(), A[:, k, :].copy()
                A[:, i, :] = np.where(swap[:, None], row_k, row_i)
                A[:, k, :] = np.where(swap[:, None], row_i, row_k)
                r_i, r_k = r[:, i].copy(), r[:, k].copy()
                r[:, i], r[:, k] = np.where(swap, r_k, r_i), np.where(swap, r_i, r_k)
            for i in range(k + 1, N):
                f = A[:, i, k] / A[:, k, k]
                A[:, i, k:] -= f[:, None] * A[:, k, k:]
                r[:, i] -= f * r[:, k]
        x = np.empty_like(r)
        for i in range(N - 1, -1, -1):
            acc = r[:, i].copy()
            for j in range(i + 1, N):
                acc -= A[:, i, j] * x[:, j]
            x[:, i] = acc / A[:, i, i]
    return x


ChemModelStruct = struct('pb_chem_model')


class ChemNetwork:
    """A gas-phase network: species[S] (names), elements[E] (names, 'H' among them),
    stoich[S, E] (non-negative integers: atoms of element j in species i), gibbs_temps[nT] (K,
    ascending), gibbs_over_RT[nT, S] (G°_i(T) / (R T) at 1 bar, dimensionless; read per column with
    np.interp at a layer's temperature, like the heat-capacity table of radiative_equilibrium),
    base_dex[E] (the solar abundances in dex, H = 12).

    ValueError for: rank(stoich) < E, an element no species holds, a species with no element, no H
    among the elements, ions or an electron 'element', a table that is not finite or whose
    temperatures do not ascend, more than min(64, the atmosphere's species limit) species, E > 8."""

    def __init__(self, species, elements, stoich, gibbs_temps, gibbs_over_RT, base_dex):
        self.species = [str(s) for s in species]
        self.elements = [str(e) for e in elements]
        S, E = self.nspecies, self.nelements = len(self.species), len(self.elements)
        limit = _species_limit()
        if not 1 <= S <= limit or len(set(self.species)) != S:
            raise ValueError(f'species: 1 ... {limit} distinct names, got {S}: {self.species}')
        if not 1 <= E <= MAX_ELEMENTS or len(set(self.elements)) != E:
            raise ValueError(f'elements: 1 ... {MAX_ELEMENTS} distinct names, got {self.elements}')
        for e in self.elements:
            if e.lower().rstrip('-') == 'e' or e[-1] in '+-':
                raise ValueError(f"elements: '{e}': ions and electrons are not supported")
        for s in self.species:
            if s[-1] in '+-' or s.lower() in ('e', 'e-'):
                raise ValueError(f"species '{s}': ions and electrons are not supported")
        if 'H' not in self.elements:
            raise ValueError(f"elements: no 'H' among {self.elements} (abundances are relative "
                             'to hydrogen)')
        stoich = np.asarray(stoich)
        if stoich.shape != (S, E):
            raise ValueError(f'stoich must have shape {(S, E)}, got {stoich.shape}')
        if not np.all(np.isfinite(stoich)) or np.any(stoich < 0) or \
                np.any(stoich != np.round(stoich)):
            raise ValueError('stoich must hold non-negative integers (ions are not supported)')
        self.stoich = np.ascontiguousarray(stoich, np.int32)
        for j, e in enumerate(self.elements):
            if not np.any(self.stoich[:, j]):
                raise ValueError(f"element '{e}' is in no species")
        for i, s in enumerate(self.species):
            if not np.any(self.stoich[i]):
                raise ValueError(f"species '{s}' holds no element")
        if np.linalg.matrix_rank(self.stoich.astype(float)) < E:
            raise ValueError(f'stoich has rank {np.linalg.matrix_rank(self.stoich.astype(float))} '
                             f'< {E} elements: the element balances are not independent')
        self.gibbs_temps = np.ascontiguousarray(gibbs_temps, float)
        self.gibbs_over_RT = np.ascontiguousarray(gibbs_over_RT, float)
        nT = len(self.gibbs_temps)
        if self.gibbs_temps.ndim != 1 or nT < 1 or self.gibbs_over_RT.shape != (nT, S):
            raise ValueError(f'gibbs_over_RT must have shape (len(gibbs_temps), {S}), got '
                             f'{self.gibbs_over_RT.shape} for {self.gibbs_temps.shape} temperatures')
        if not np.all(np.isfinite(self.gibbs_temps)) or not np.all(np.isfinite(self.gibbs_over_RT)):
            raise ValueError('gibbs_temps and gibbs_over_RT must be finite')
        if np.any(np.diff(self.gibbs_temps) <= 0) or self.gibbs_temps[0] <= 0:
            raise ValueError('gibbs_temps must be positive and ascending')
        self.base_dex = np.ascontiguousarray(base_dex, float)
        if self.base_dex.shape != (E,) or not np.all(np.isfinite(self.base_dex)):
            raise ValueError(f'base_dex must hold {E} finite values, got {self.base_dex}')
        self.ihydrogen = self.elements.index('H')
        self.is_metal = np.array([e not in ('H', 'He') for e in self.elements])
        self._dev = None

    # ------------------------------------------------------------------------ abundances
    def element_index(self, name):
        if name not in self.elements:
            raise ValueError(f"element '{name}' is not in the network ({self.elements})")
        return self.elements.index(name)

    def ratio_elements(self, name):
        """'C/O' (or the reference's key 'C_O') -> the indices of C and O."""
        sep = '/' if '/' in name else '_'
        if name.count(sep) != 1:
            raise ValueError(f"element ratio '{name}': the format is X/Y")
        x, y = name.split(sep)
        return self.element_index(x), self.element_index(y)

    def element_abundances_host(self, metallicity=None, e_scale=None, e_ratio=None):
        """b[E], the elemental abundances relative to H, by the rule of the reference's
        documentation (docs/atmosphere_modeling.rst, the vmr_vars table):
          1. start from base_dex;
          2. every element but H and He gets + metallicity ([M/H]; None: 0);
          3. e_scale {X: [X/H]} sets dex[X] = base_dex[X] + value, overriding the metallicity;
          4. e_ratio {'X/Y': value}, after those and in the mapping's order, sets
             dex[X] = dex[Y] + log10(value);
          5. b_j = 10**(dex_j - dex_H).
        None when the walker is to be rejected: a ratio <= 0 (or NaN), or an abundance that is
        not finite and positive."""
        dex = self.base_dex.copy()
        if metallicity is not None:
            dex[self.is_metal] = self.base_dex[self.is_metal] + np.float64(metallicity)
        for name, value in (e_scale or {}).items():
            j = self.element_index(name)
            dex[j] = self.base_dex[j] + np.float64(value)
        for name, value in (e_ratio or {}).items():
            x, y = self.ratio_elements(name)
            if not value > 0.0:
                return None
            dex[x] = dex[y] + np.log10(np.float64(value))
        with np.errstate(all='ignore'):
            b = np.float64(10.0)**(dex - dex[self.ihydrogen])
        if not np.all(np.isfinite(b) & (b > 0.0)):
            return None
        return b

    # ------------------------------------------------------------------------ equilibrium
    def gibbs_at(self, temp):
        """g[len(temp), S]: np.interp of every column of the table."""
        temp = np.atleast_1d(np.asarray(temp, float))
        return np.stack([np.interp(temp, self.gibbs_temps, self.gibbs_over_RT[:, i])
                         for i in range(self.nspecies)], axis=1)

    def equilibrium_host(self, temp, pressure, b, tolerance=TOLERANCE):
        """temp[L] (K), pressure[L] (bar), b[E] (element_abundances_host; None: a rejected walker)
        -> vmr[L, S], iterations[L], status[L].  status is the iteration count of a converged cell
        or a negative STATUS_*; a cell with a negative status has zeros in vmr and iterated
        nothing (STATUS_NOT_CONVERGED: MAX_ITERATIONS).  Every cell is solved from the same cold
        start n_i = 0.1 / S, n = 0.1, so it depends on nothing but its own inputs."""
        temp = np.atleast_1d(np.asarray(temp, float))
        pressure = np.atleast_1d(np.asarray(pressure, float))
        L, S, E = len(temp), self.nspecies, self.nelements
        if temp.shape != (L,) or pressure.shape != (L,):
            raise ValueError(f'temp and pressure must have one shape (L,), got {temp.shape} and '
                             f'{pressure.shape}')
        if np.any(~(pressure > 0)):
            raise ValueError('pressure must be positive')
        vmr = np.zeros((L, S))
        iterations = np.zeros(L, np.int32)
        status = np.zeros(L, np.int32)
        status[~(temp > 0.0)] = STATUS_REJECTED
        if b is None:
            status[status == 0] = STATUS_RATIO
        else:
            b = np.asarray(b, float)
            if b.shape != (E,):
                raise ValueError(f'b must have shape {(E,)}, got {b.shape}')
        outside = ~((temp >= self.gibbs_temps[0]) & (temp <= self.gibbs_temps[-1]))
        status[(status == 0) & outside] = STATUS_TEMPERATURE
        live = np.where(status == 0)[0]
        if live.size:
            v, it, ok = self._newton(self.gibbs_at(temp[live]), np.log(pressure[live]), b,
                                     tolerance)
            vmr[live] = np.where(ok[:, None], v, 0.0)
            iterations[live] = it
            status[live] = np.where(ok, it, STATUS_NOT_CONVERGED)
        return vmr, iterations, status

    def _newton(self, g, lnp, b, tolerance):
        """The iteration of the module docstring on c cells at once (each on its own; a converged
        cell is left alone): g[c, S], lnp[c] -> vmr[c, S], iterations[c], converged[c]."""
        a = self.stoich.astype(float)
        c, S, E = len(lnp), self.nspecies, self.nelements
        ln_ni = np.full((c, S), np.log(0.1 / S))
        ln_n = np.full(c, np.log(0.1))
        iterations = np.zeros(c, np.int32)
        converged = np.zeros(c, bool)
        with np.errstate(all='ignore'):
            for it in range(1, MAX_ITERATIONS + 1):
                idx = np.where(~converged)[0]
                if not idx.size:
                    break
                li, ln = ln_ni[idx], ln_n[idx]
                ni, n = np.exp(li), np.exp(ln)
                mu = ((g[idx] + li) - ln[:, None]) + lnp[idx][:, None]
                an = a[None, :, :] * ni[:, :, None]                       # a_ik n_i
                A = np.empty((len(idx), E + 1, E + 1))
                A[:, :E, :E] = np.einsum('sk,csj->ckj', a, an)
                col = an.sum(axis=1)
                A[:, :E, E] = col
                A[:, E, :E] = col
                sn = ni.sum(axis=1)
                A[:, E, E] = sn - n
                r = np.empty((len(idx), E + 1))
                r[:, :E] = (b - col) + np.einsum('csk,cs->ck', an, mu)
                r[:, E] = (n - sn) + (ni * mu).sum(axis=1)
                x = gauss_solve(A, r)
                dln_n = x[:, E]
                dln_ni = (-mu + dln_n[:, None]) + x[:, :E] @ a.T
                rel = li - ln[:, None]                                    # ln(n_i / n)
                major = ni / n[:, None] > _MINOR
                step = np.where(major, np.abs(dln_ni), 0.0).max(axis=1)
                l1 = 2.0 / np.fmax(5.0 * np.abs(dln_n), step)
                minor = ~major & (dln_ni >= 0.0)
                q = np.abs((-rel - _LN_MINOR) / (dln_ni - dln_n[:, None]))
                l2 = np.fmin.reduce(np.where(minor, q, np.inf), axis=1)
                lam = np.fmin(1.0, np.fmin(l1, l2))
                ln_ni[idx] = li + lam[:, None] * dln_ni
                ln_n[idx] = ln + lam * dln_n
                iterations[idx] = it
                small = np.all((ni * np.abs(dln_ni)) / sn[:, None] < tolerance, axis=1)
                done = (lam == 1.0) & small & (np.abs(dln_n) < tolerance)
                converged[idx] = done
            ni = np.exp(ln_ni)
            vmr = ni / ni.sum(axis=1)[:, None]
        return vmr, iterations, converged

    def hybrid_host(self, vmr, species, value):
        """The column of a free log10(VMR) on top of the equilibrium vmr[L, S] (the reference's
        hybrid_vmr, vmr_models.py:40-57): clip(10**value, 0, max_vmr) with max_vmr the smallest,
        over the species' elements j, of (sum_i vmr_i a_ij) / a_species,j -- the species cannot
        hold more of an element than the mixture has.  Nothing is renormalised."""
        k = self.species.index(species)
        vmr = np.asarray(vmr, float)
        caps = [(vmr * self.stoich[:, j]).sum(axis=1) / self.stoich[k, j]
                for j in range(self.nelements) if self.stoich[k, j]]
        max_vmr = np.min(caps, axis=0)
        return np.clip(np.float64(10.0)**value, 0.0, max_vmr)

    # ----------------------------------------------------------------------------- device
    def device_arrays(self):
        from ._device import dev, require_gpu
        import torch
        require_gpu()
        if self._dev is None:
            self._dev = dict(temps=dev(self.gibbs_temps), gibbs=dev(self.gibbs_over_RT),
                             stoich=torch.tensor(self.stoich, dtype=torch.int32, device='cuda'))
        return self._dev

    def model_struct(self, nlayers, npar, par_metal=-1, scales=(), ratios=(), hybrids=()):
        """The pb_chem_model of this network with its scalar fields set (device pointers: null).
        par_metal: the column of [M/H] or -1; scales: (element index, column) per [X/H]; ratios:
        (index of X, index of Y, column) per X/Y, in model order; hybrids: (species index,
        column) per free log10(VMR)."""
        if len(scales) > MAX_ELEMENTS or len(ratios) > MAX_ELEMENTS or len(hybrids) > MAX_HYBRID:
            raise ValueError(f'at most {MAX_ELEMENTS} [X/H], {MAX_ELEMENTS} X/Y and {MAX_HYBRID} '
                             'hybrid models')
        st = ChemModelStruct()
        st.nspecies, st.nelements, st.ntemps = self.nspecies, self.nelements, len(self.gibbs_temps)
        st.nlayers, st.npar, st.ihydrogen = int(nlayers), int(npar), self.ihydrogen
        for j in range(self.nelements):
            st.base_dex[j], st.is_metal[j] = self.base_dex[j], int(self.is_metal[j])
        st.par_metal = int(par_metal)
        st.nscale, st.nratio, st.nhybrid = len(scales), len(ratios), len(hybrids)
        for k, (j, col) in enumerate(scales):
            st.scale_element[k], st.scale_par[k] = j, col
        for k, (x, y, col) in enumerate(ratios):
            st.ratio_num[k], st.ratio_den[k], st.ratio_par[k] = x, y, col
        for k, (i, col) in enumerate(hybrids):
            st.hybrid_species[k], st.hybrid_par[k] = i, col
        st.max_iterations, st.tolerance = MAX_ITERATIONS, TOLERANCE
        return st

    def bound_struct(self, pressure_d, npar, **columns):
        """model_struct with the device pointers of this network and of pressure_d[L] (bar)."""
        d = self.device_arrays()
        st = self.model_struct(pressure_d.shape[0], npar, **columns)
        st.gibbs_temps_d, st.gibbs_d = d['temps'].data_ptr(), d['gibbs'].data_ptr()
        st.stoich_d, st.pressure_d = d['stoich'].data_ptr(), pressure_d.data_ptr()
        return st


def equilibrium_vmr(net, temps, pressure, params=None, par_metal=-1, scales=(), ratios=(),
                    hybrids=(), out=None):
    """pb_equilibrium_vmr at its boundary: temps[nw, L] and pressure[L] (float64 device tensors),
    params[nw, npar] (or None when no column is named) -> (vmr[nw, L, S], status[nw, L] int32),
    written into `out` when given.  One launch, nothing read back."""
    import torch
    from ._capi import call
    for name, t, dim in (('temps', temps, 2), ('pressure', pressure, 1)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != dim or \
                not t.is_cuda or not t.is_contiguous():
            raise ValueError(f'equilibrium_vmr: {name} must be a contiguous float64 device tensor '
                             f'of {dim} dimensions')
    nw, L = temps.shape
    if pressure.shape[0] != L:
        raise ValueError(f'equilibrium_vmr: {L} layers of temps, {pressure.shape[0]} pressures')
    npar = 0
    if params is not None:
        if not isinstance(params, torch.Tensor) or params.dtype != torch.float64 or \
                params.dim() != 2 or params.shape[0] != nw or not params.is_cuda or \
                not params.is_contiguous():
            raise ValueError(f'equilibrium_vmr: params must be a contiguous float64 device tensor '
                             f'of shape ({nw}, npar)')
        npar = params.shape[1]
    st = net.bound_struct(pressure, npar, par_metal=par_metal, scales=scales, ratios=ratios,
                          hybrids=hybrids)
    if out is None:
        out = (torch.empty((nw, L, net.nspecies), dtype=torch.float64, device=temps.device),
               torch.empty((nw, L), dtype=torch.int32, device=temps.device))
    vmr, status = out
    if tuple(vmr.shape) != (nw, L, net.nspecies) or vmr.dtype != torch.float64 or \
            tuple(status.shape) != (nw, L) or status.dtype != torch.int32 or \
            not vmr.is_contiguous() or not status.is_contiguous():
        raise ValueError(f'equilibrium_vmr: out must be (float64 {(nw, L, net.nspecies)}, int32 '
                         f'{(nw, L)}), contiguous')
    call('pb_equilibrium_vmr', C.byref(st), temps.data_ptr(),
         None if params is None else params.data_ptr(), nw, vmr.data_ptr(), status.data_ptr(),
         torch.cuda.current_stream().cuda_stream)
    return vmr, status
