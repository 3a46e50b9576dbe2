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

Inside the radiative-equilibrium loop (radeq.RadiativeEquilibrium(chemistry=...)) a cell's
temperature moves by little between two solves, so CarriedEquilibrium (pb_radeq_equilibrium) starts
from the iterate of the previous one; equilibrium_host(start=...) is its host form and TOL_ALL the
extra convergence test a carried start needs.

Ions and electrons: ChemNetwork(..., charges=[S]) gives every species its charge; the electron is a
species 'e-' with an all-zero stoich row and charge -1, and the charge never enters stoich.  The
charge balance sum_i q_i n_i = 0 is one more row of the system (net.balance = [stoich | charges],
its b is 0), which then has order E + 2.  Allowing that row is not enough (profiles/
chemistry_ions.md): from the cold start an ion moves by about one unit of ln n per iteration, and
the convergence test above, which weighs a step by n_i, does not see the charge balance of trace
ions at all.  So the cold solve takes three steps:
    1. the neutral species alone, from the cold start of their sub-network (its statements and
       bits), which leaves the element potentials pi of its last solve;
    2. every charged species is seeded in logarithms: ln n_i = t_i + q_i pi_q with
       t_i = ln n - g_i - ln p + sum_j a_ij pi_j and pi_q = (LSE- - LSE+) / 2, LSE the log-sum-exp
       of t over the species of one sign (exact for charges +-1 while the ions are trace);
    3. the full system from there, converged when the test above holds AND |dln n_i| < TOL_ALL for
       every charged species.  Where sum_i q_i^2 n_i == 0 (every ion has underflowed) the charge
       row and column of that iteration are an identity row with right-hand side 0 and the
       charged species keep their ln n_i.
iterations and status are the sum of steps 1 and 3, each capped at MAX_ITERATIONS.  A carried start
goes straight to step 3.  charges=None or all zeros is the neutral network: the statements above,
every refusal and every bit unchanged.

Out of scope: condensates, networks above 64 species (profiles/chemistry.md).
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
# max_i |dln n_i| below which a solve from a carried iterate has converged.  The test above weighs
# a step by n_i, so from a neighbouring solution it can pass after ONE step, with the trace species
# still off by the first-order error of the major ones (a factor 2.3 measured); bounding every
# species' own step removes that.  1e-6 and 1e-11 give the same result
# (profiles/radeq_chemistry.md).
TOL_ALL = 1.0e-9
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
    temperatures do not ascend, more than min(64, the atmosphere's species limit) species, E > 8.

    charges[S] (integers; None or all zeros: a neutral network, everything above as it is): the
    charge of every species.  Names ending in '+' or '-' and 'e-' are then taken, and a species
    holds an element or a charge.  ValueError for: charged species of one sign only, an element
    that no neutral species holds, rank(stoich of the neutral species) < E, rank([stoich |
    charges]) < E + 1, E > 7 (the charge balance takes one of the eight rows).  net.charges is the
    int32 array (or None), net.balance [S, E + 1] = [stoich | charges]; net.stoich stays [S, E]."""

    def __init__(self, species, elements, stoich, gibbs_temps, gibbs_over_RT, base_dex,
                 charges=None):
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
        if charges is not None:
            charges = np.asarray(charges)
            if charges.shape != (S,) or not np.all(np.isfinite(charges)) or \
                    np.any(charges != np.round(charges)):
                raise ValueError(f'charges must hold {S} integers, one per species, got '
                                 f'{charges}')
            charges = np.ascontiguousarray(charges, np.int32)
        self.charges = charges
        # all zeros is the neutral network: today's statements, refusals and bits
        self.charged = charges is not None and bool(np.any(charges))
        for s in self.species:
            if not self.charged and (s[-1] in '+-' or s.lower() in ('e', 'e-')):
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
            if not np.any(self.stoich[i]) and not (self.charged and self.charges[i]):
                raise ValueError(f"species '{s}' holds no element" +
                                 ' and no charge' * self.charged)
        if self.charged:
            self._check_charges()
        elif np.linalg.matrix_rank(self.stoich.astype(float)) < E:
            raise ValueError(f'stoich has rank {np.linalg.matrix_rank(self.stoich.astype(float))} '
                             f'< {E} elements: the element balances are not independent')
        self.balance = np.ascontiguousarray(np.column_stack(
            [self.stoich, np.zeros(S, np.int32) if charges is None else self.charges]), np.int32)
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

    def _check_charges(self):
        """What a network with ions and electrons has to hold on top (the class docstring)."""
        E, q = self.nelements, self.charges
        if E + 1 > MAX_ELEMENTS:
            raise ValueError(f'{E} elements with charges: the charge balance takes one of the '
                             f'{MAX_ELEMENTS} rows, at most {MAX_ELEMENTS - 1} elements')
        if not (np.any(q > 0) and np.any(q < 0)):
            raise ValueError('charges: charged species of both signs must be present (got '
                             f'{[s for s, c in zip(self.species, q) if c]}): no charge balance '
                             'otherwise')
        neutral = self.stoich[q == 0].astype(float)
        for j, e in enumerate(self.elements):
            if not np.any(neutral[:, j]):
                raise ValueError(f"element '{e}' is in no neutral species (the neutral "
                                 'sub-network is solved first)')
        full = np.column_stack([self.stoich, q]).astype(float)
        rank = np.linalg.matrix_rank(full)
        if rank < E + 1:
            raise ValueError(f'[stoich | charges] has rank {rank} < {E} elements + 1: the charge '
                             'balance is not independent of the element balances')
        rank = np.linalg.matrix_rank(neutral)
        if rank < E:
            raise ValueError(f'the stoich of the neutral species has rank {rank} < {E} elements: '
                             'the element balances are not independent')

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

    def equilibrium_host(self, temp, pressure, b, tolerance=TOLERANCE, start=None,
                         tol_all=TOL_ALL):
        """temp[L] (K), pressure[L] (bar), b[E] (element_abundances_host; None: a rejected walker)
        -> vmr[L, S], iterations[L], status[L].  status is the iteration count of a converged cell
        or a negative STATUS_*; a cell with a negative status has zeros in vmr and iterated
        nothing (STATUS_NOT_CONVERGED: MAX_ITERATIONS).  Every cell is solved from the same cold
        start n_i = 0.1 / S, n = 0.1, so it depends on nothing but its own inputs.  (A network
        with charges: the three steps of the module docstring, iterations their sum.)

        start: the host form of pb_radeq_equilibrium, which also returns the iterate, a fourth
        element (ln_ni[L, S], ln_n[L]).  'cold': as above.  (ln_ni[L, S], ln_n[L]), the iterate an
        earlier call returned: a cell starts from it and has converged when the test above holds
        AND max_i |dln n_i| < tol_all (module docstring); a cell whose start is not finite, or that
        does not converge from it, is solved from the cold start, with the cold result's bits;
        iterations and status then count the cold solve.  A cell with a negative status returns
        its start unchanged (the cold start under 'cold')."""
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
        if start is None:
            if live.size:
                v, it, ok = self._newton(self.gibbs_at(temp[live]), np.log(pressure[live]), b,
                                         tolerance)
                vmr[live] = np.where(ok[:, None], v, 0.0)
                iterations[live] = it
                status[live] = np.where(ok, it, STATUS_NOT_CONVERGED)
            return vmr, iterations, status
        if isinstance(start, str):
            if start != 'cold':
                raise ValueError(f"start {start!r}: 'cold' or (ln_ni[L, S], ln_n[L])")
            ln_ni, ln_n = self._cold_start(L)
            warm = np.zeros(L, bool)
        else:
            ln_ni, ln_n = (np.array(v, float) for v in start)
            if ln_ni.shape != (L, S) or ln_n.shape != (L,):
                raise ValueError(f'start must have shapes {(L, S)} and {(L,)}, got {ln_ni.shape} '
                                 f'and {ln_n.shape}')
            warm = np.all(np.isfinite(ln_ni), axis=1) & np.isfinite(ln_n)
        if live.size:
            g, lnp = self.gibbs_at(temp[live]), np.log(pressure[live])
            ok = np.zeros(len(live), bool)
            it = np.zeros(len(live), np.int32)
            v = np.zeros((len(live), S))
            li, ln = ln_ni[live].copy(), ln_n[live].copy()
            first = np.where(warm[live])[0]
            if first.size:
                v[first], it[first], ok[first], li[first], ln[first] = self._newton(
                    g[first], lnp[first], b, tolerance, (li[first], ln[first]), tol_all)
            again = np.where(~ok)[0]
            if again.size:
                v[again], it[again], ok[again], li[again], ln[again] = self._newton(
                    g[again], lnp[again], b, tolerance, iterate=True)
            good = live[ok]
            vmr[good], ln_ni[good], ln_n[good] = v[ok], li[ok], ln[ok]
            iterations[live] = it
            status[live] = np.where(ok, it, STATUS_NOT_CONVERGED)
        return vmr, iterations, status, (ln_ni, ln_n)

    def _cold_start(self, c):
        """(ln_ni[c, S], ln_n[c]) every cell starts from: n_i = 0.1 / S, n = 0.1."""
        return np.full((c, self.nspecies), np.log(0.1 / self.nspecies)), np.full(c, np.log(0.1))

    def _newton(self, g, lnp, b, tolerance, start=None, tol_all=None, iterate=False):
        """The iteration of the module docstring on c cells at once (each on its own; a converged
        cell is left alone): g[c, S], lnp[c] -> vmr[c, S], iterations[c], converged[c].  start
        (ln_ni[c, S], ln_n[c]): from that iterate instead of the cold start, and the iterate is
        returned too (ln_ni, ln_n behind the three; iterate=True: also from the cold start);
        tol_all: converged only when also max_i |dln n_i| < tol_all.  With charges the cold start
        is the three steps of the module docstring, a given start goes straight to the third."""
        a = self.stoich.astype(float)
        c = len(lnp)
        with np.errstate(all='ignore'):
            if not self.charged:
                ln_ni, ln_n = self._cold_start(c) if start is None else \
                    (np.array(start[0], float), np.array(start[1], float))
                ln_ni, ln_n, iterations, converged, _ = self._iterate(
                    a, b, g, lnp, tolerance, ln_ni, ln_n, tol_all)
            else:
                ions = self.charges != 0
                full, b_full = self.balance.astype(float), np.append(np.asarray(b, float), 0.0)
                if start is not None:
                    ln_ni, ln_n, iterations, converged, _ = self._iterate(
                        full, b_full, g, lnp, tolerance, np.array(start[0], float),
                        np.array(start[1], float), tol_all, ions)
                else:
                    ln_ni, ln_n, iterations, converged = self._cold_ions(
                        a, full, b, b_full, g, lnp, tolerance, ions)
            ni = np.exp(ln_ni)
            vmr = ni / ni.sum(axis=1)[:, None]
        if start is None and not iterate:
            return vmr, iterations, converged
        return vmr, iterations, converged, ln_ni, ln_n

    def _cold_ions(self, a, full, b, b_full, g, lnp, tolerance, ions):
        """The cold solve of a network with charges (module docstring): the neutral sub-network,
        the charged species seeded from its element potentials, then the full system."""
        c, S = g.shape
        neutral = ~ions
        count = int(neutral.sum())
        # 1: exactly the sub-network of the neutral species, from ITS cold start
        sub_ni, ln_n, iterations, converged, pi = self._iterate(
            a[neutral], b, g[:, neutral], lnp, tolerance,
            np.full((c, count), np.log(0.1 / count)), np.full(c, np.log(0.1)))
        ln_ni = np.zeros((c, S))
        ln_ni[:, neutral] = sub_ni
        # 2: ln n_i = ln n - g_i - ln p + sum_j a_ij pi_j + q_i pi_q, in logarithms throughout
        q = self.charges[ions].astype(float)
        t = ((ln_n[:, None] - g[:, ions]) - lnp[:, None]) + pi @ a[ions].T

        def lse(mask):
            top = np.max(np.where(mask, t, -np.inf), axis=1)
            return top + np.log(np.sum(np.where(mask, np.exp(t - top[:, None]), 0.0), axis=1))
        pi_q = 0.5 * (lse(q < 0.0) - lse(q > 0.0))
        ln_ni[:, ions] = t + q * pi_q[:, None]
        # 3: the full system of order E + 2 on the cells the first step solved
        ok = np.where(converged)[0]
        if ok.size:
            ln_ni[ok], ln_n[ok], more, converged[ok], _ = self._iterate(
                full, b_full, g[ok], lnp[ok], tolerance, ln_ni[ok], ln_n[ok], None, ions)
            iterations[ok] += more
        return ln_ni, ln_n, iterations, converged

    def _iterate(self, a, b, g, lnp, tolerance, ln_ni, ln_n, tol_all=None, ions=None):
        """The Newton loop proper on the balance matrix a[S, E] (stoich, or [stoich | charges]
        with ions[S] marking the charged species and b's last entry 0) from the iterate
        (ln_ni[c, S], ln_n[c]), both updated in place -> ln_ni, ln_n, iterations[c], converged[c],
        pi[c, E] (the potentials of each cell's last solve)."""
        c, S = g.shape
        E = a.shape[1]
        iterations = np.zeros(c, np.int32)
        converged = np.zeros(c, bool)
        pi = np.zeros((c, E))
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
            if ions is not None:
                # sum_i q_i^2 n_i == 0: every ion has underflowed, the charge row and column are
                # zeros; an identity row in their place, and the ions keep their ln n_i
                drop = A[:, E - 1, E - 1] == 0.0
                A[drop, E - 1, :] = 0.0
                A[drop, :, E - 1] = 0.0
                A[drop, E - 1, E - 1] = 1.0
                r[drop, E - 1] = 0.0
                held = drop[:, None] & ions[None, :]
            x = gauss_solve(A, r)
            dln_n = x[:, E]
            dln_ni = (-mu + dln_n[:, None]) + x[:, :E] @ a.T
            if ions is not None:
                dln_ni = np.where(held, 0.0, dln_ni)
            rel = li - ln[:, None]                                    # ln(n_i / n)
            major = ni / n[:, None] > _MINOR
            step = np.where(major, np.abs(dln_ni), 0.0).max(axis=1)
            l1 = 2.0 / np.fmax(5.0 * np.abs(dln_n), step)
            minor = ~major & (dln_ni >= 0.0)
            if ions is not None:
                minor &= ~held
            q = np.abs((-rel - _LN_MINOR) / (dln_ni - dln_n[:, None]))
            l2 = np.fmin.reduce(np.where(minor, q, np.inf), axis=1)
            lam = np.fmin(1.0, np.fmin(l1, l2))
            ln_ni[idx] = li + lam[:, None] * dln_ni
            ln_n[idx] = ln + lam * dln_n
            iterations[idx] = it
            pi[idx] = x[:, :E]
            small = np.all((ni * np.abs(dln_ni)) / sn[:, None] < tolerance, axis=1)
            done = (lam == 1.0) & small & (np.abs(dln_n) < tolerance)
            if tol_all is not None:
                done &= np.all(np.abs(dln_ni) < tol_all, axis=1)
            if ions is not None:
                # the weighted test does not see a trace species, hence not the charge balance
                done &= np.all(np.abs(dln_ni[:, ions]) < TOL_ALL, axis=1)
            converged[idx] = done
        return ln_ni, ln_n, iterations, converged, pi

    def hybrid_host(self, vmr, species, value):
        """The column of a free log10(VMR) on top of the equilibrium vmr[L, S] (the reference's
        hybrid_vmr, vmr_models.py:40-57): clip(10**value, 0, max_vmr) with max_vmr the smallest,
        over the species' elements j, of (sum_i vmr_i a_ij) / a_species,j -- the species cannot
        hold more of an element than the mixture has.  Nothing is renormalised."""
        k = self.species.index(species)
        self.refuse_charged_hybrid(k)
        vmr = np.asarray(vmr, float)
        caps = [(vmr * self.stoich[:, j]).sum(axis=1) / self.stoich[k, j]
                for j in range(self.nelements) if self.stoich[k, j]]
        max_vmr = np.min(caps, axis=0)
        return np.clip(np.float64(10.0)**value, 0.0, max_vmr)

    def refuse_charged_hybrid(self, k):
        if self.charged and self.charges[k]:
            raise ValueError(f"hybrid model on '{self.species[k]}': a charged species takes no "
                             'free VMR (the charge balance would not hold)')

    # ----------------------------------------------------------------------------- device
    def device_arrays(self):
        from ._device import dev, require_gpu
        import torch
        require_gpu()
        if self._dev is None:
            self._dev = dict(temps=dev(self.gibbs_temps), gibbs=dev(self.gibbs_over_RT),
                             stoich=torch.tensor(self.stoich, dtype=torch.int32, device='cuda'))
            if self.charged:
                self._dev['charges'] = torch.tensor(self.charges, dtype=torch.int32,
                                                    device='cuda')
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
            if 0 <= i < self.nspecies:
                self.refuse_charged_hybrid(i)
            st.hybrid_species[k], st.hybrid_par[k] = i, col
        st.max_iterations, st.tolerance = MAX_ITERATIONS, TOLERANCE
        return st

    def bound_struct(self, pressure_d, npar, **columns):
        """model_struct with the device pointers of this network and of pressure_d[L] (bar)."""
        d = self.device_arrays()
        st = self.model_struct(pressure_d.shape[0], npar, **columns)
        st.gibbs_temps_d, st.gibbs_d = d['temps'].data_ptr(), d['gibbs'].data_ptr()
        st.stoich_d, st.pressure_d = d['stoich'].data_ptr(), pressure_d.data_ptr()
        st.charge_d = d['charges'].data_ptr() if self.charged else None
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


RadeqChemStruct = struct('pb_radeq_chem')


class CarriedEquilibrium:
    """The buffers of pb_radeq_equilibrium for nw profiles of L layers on pressure_d[L] (bar): the
    carried iterate (ln_ni, ln_n), the outputs vmr[nw, L, S], mm[nw, L], status[nw, L] and the
    failure counts failures[nw, L] (zeroed here), device tensors all.  params[nw, npar] (or None)
    and the columns par_metal, scales, ratios as in equilibrium_vmr; hybrid models are refused
    (the carried iterate is that of the equilibrium alone)."""

    def __init__(self, net, nw, pressure_d, mol_mass, params=None, par_metal=-1, scales=(),
                 ratios=(), hybrids=(), tol_all=TOL_ALL):
        import torch
        from ._device import dev
        if len(hybrids):
            raise ValueError(f'{len(hybrids)} hybrid models: pb_radeq_equilibrium carries the '
                             'iterate of the equilibrium alone and takes none')
        L, S = pressure_d.shape[0], net.nspecies
        mol_mass = np.asarray(mol_mass, float)
        if mol_mass.shape != (S,):
            raise ValueError(f'mol_mass must have shape ({S},), got {mol_mass.shape}')
        if not tol_all > 0.0:
            raise ValueError(f'tol_all = {tol_all}: must be > 0')
        npar = 0
        if params is not None:
            if not isinstance(params, torch.Tensor) or params.dtype != torch.float64 or \
                    params.dim() != 2 or params.shape[0] != nw or not params.is_cuda or \
                    not params.is_contiguous():
                raise ValueError('params must be a contiguous float64 device tensor of shape '
                                 f'({nw}, npar)')
            npar = params.shape[1]
        self.net, self.nw, self.params, self.pressure = net, nw, params, pressure_d
        self.model = net.bound_struct(pressure_d, npar, par_metal=par_metal, scales=scales,
                                      ratios=ratios)

        def new(*shape, dtype=torch.float64, fill=float('nan')):
            return torch.full(shape, fill, dtype=dtype, device=pressure_d.device)
        self.ln_ni, self.ln_n = new(nw, L, S), new(nw, L)
        self.vmr, self.mm = new(nw, L, S), new(nw, L)
        self.status = new(nw, L, dtype=torch.int32, fill=0)
        self.failures = new(nw, L, dtype=torch.int32, fill=0)
        self.mol_mass = dev(mol_mass)
        self.state = RadeqChemStruct()
        for name in ('ln_ni', 'ln_n', 'vmr', 'mm', 'mol_mass', 'status', 'failures'):
            setattr(self.state, name + '_d', getattr(self, name).data_ptr())
        self.state.tol_all = float(tol_all)

    def solve(self, temps, warm):
        """One launch at temps[nw, L] (a contiguous float64 device tensor); nothing read back."""
        import torch
        from ._capi import call
        if not isinstance(temps, torch.Tensor) or temps.dtype != torch.float64 or \
                tuple(temps.shape) != (self.nw, self.pressure.shape[0]) or not temps.is_cuda or \
                not temps.is_contiguous():
            raise ValueError('temps must be a contiguous float64 device tensor of shape '
                             f'{(self.nw, self.pressure.shape[0])}')
        call('pb_radeq_equilibrium', C.byref(self.model), temps.data_ptr(),
             None if self.params is None else self.params.data_ptr(), self.nw, int(bool(warm)),
             C.byref(self.state), torch.cuda.current_stream().cuda_stream)
