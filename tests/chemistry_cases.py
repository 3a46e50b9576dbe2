"""Shared cases of the equilibrium-chemistry tests (CPU and GPU): the 16-species C-H-N-O-He
network with a synthetic Gibbs table, the 28-point (T, p) grid, small networks with closed forms,
a network padded to the species limit, and the two solver-independent optimality measures."""
import numpy as np

SPECIES = ['H2', 'H', 'He', 'H2O', 'CH4', 'CO', 'CO2', 'NH3', 'N2', 'HCN', 'C2H2', 'OH', 'O', 'C',
           'N', 'O2']
ELEMENTS = ['H', 'He', 'C', 'N', 'O']
STOICH = np.array([
    # H He  C  N  O
    [2, 0, 0, 0, 0],    # H2
    [1, 0, 0, 0, 0],    # H
    [0, 1, 0, 0, 0],    # He
    [2, 0, 0, 0, 1],    # H2O
    [4, 0, 1, 0, 0],    # CH4
    [0, 0, 1, 0, 1],    # CO
    [0, 0, 1, 0, 2],    # CO2
    [3, 0, 0, 1, 0],    # NH3
    [0, 0, 0, 2, 0],    # N2
    [1, 0, 1, 1, 0],    # HCN
    [2, 0, 2, 0, 0],    # C2H2
    [1, 0, 0, 0, 1],    # OH
    [0, 0, 0, 0, 1],    # O
    [0, 0, 1, 0, 0],    # C
    [0, 0, 0, 1, 0],    # N
    [0, 0, 0, 0, 2],    # O2
])
MASS = np.array([2.01588, 1.00794, 4.002602, 18.01528, 16.0425, 28.0101, 44.0095, 17.03052,
                 28.0134, 27.02534, 26.03728, 17.00734, 15.9994, 12.0107, 14.0067, 31.9988])
# synthetic thermochemistry: g_i(T) = (h_i - T s_i) / (8.314 T)
H_FORM = np.array([0, 218, 0, -242, -75, -110, -393, -46, 0, 135, 227, 39, 249, 717, 473, 0]) * 1e3
S_ENT = np.array([130, 115, 126, 189, 186, 198, 214, 193, 192, 202, 201, 184, 161, 158, 153, 205.0])
B = np.array([1.0, 0.085, 2.7e-4, 6.8e-5, 4.9e-4])          # H, He, C, N, O
BASE_DEX = 12.0 + np.log10(B)
GRID_T = [300.0, 600.0, 1000.0, 1500.0, 2500.0, 4000.0, 6000.0]
GRID_P = [1e-8, 1e-4, 1.0, 100.0]
GRID = [(t, p) for t in GRID_T for p in GRID_P]
# a table on which g is linear in 1/T only between nodes: the nodes include every grid
# temperature, so that np.interp returns g_i(T) itself there
TABLE_T = np.array(sorted(set(GRID_T) | {200.0, 2000.0, 3000.0, 5000.0, 6500.0}))


def gibbs(temps, h=H_FORM, s=S_ENT):
    temps = np.asarray(temps, float)
    return (h[None, :] - temps[:, None] * s[None, :]) / (8.314 * temps[:, None])


def network(ch):
    """The 16-species network of the module docstring."""
    return ch.ChemNetwork(SPECIES, ELEMENTS, STOICH, TABLE_T, gibbs(TABLE_T), BASE_DEX)


def hydrogen_network(ch, with_helium=False):
    """H2 <=> 2 H (S = 2, E = 1), optionally with an inert He."""
    species, elements = ['H2', 'H'], ['H']
    stoich = [[2], [1]]
    h, s = H_FORM[:2], S_ENT[:2]
    dex = [12.0]
    if with_helium:
        species, elements = species + ['He'], elements + ['He']
        stoich = [[2, 0], [1, 0], [0, 1]]
        h, s = H_FORM[:3], S_ENT[:3]
        dex = [12.0, BASE_DEX[1]]
    return ch.ChemNetwork(species, elements, stoich, TABLE_T, gibbs(TABLE_T, h, s), dex)


def hydrogen_closed_form(temp, pressure):
    """x_H of H2 <=> 2 H: x_H^2 / (1 - x_H) = K, K = exp(g_H2 - 2 g_H) / p."""
    g = gibbs([temp], H_FORM[:2], S_ENT[:2])[0]
    K = np.exp(g[0] - 2.0 * g[1]) / pressure
    return (-K + np.sqrt(K * K + 4.0 * K)) / 2.0


def padded_network(ch, nspecies):
    """The 16-species network padded to nspecies: inert noble-gas-like species of one new element
    each up to E = 8 (Ne, Ar, Kr), then their dimers and mixed clusters."""
    new = ['Ne', 'Ar', 'Kr']
    species, elements = list(SPECIES), list(ELEMENTS) + new
    rows = [list(r) + [0, 0, 0] for r in STOICH]
    h, s = list(H_FORM), list(S_ENT)
    # abundant on purpose: the solver's convergence test weighs a step by n_i, so an element's
    # balance is converged to tolerance / b_k only (profiles/chemistry.md)
    dex = list(BASE_DEX) + [10.9, 10.5, 10.1]
    clusters = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0),
                (1, 0, 1), (0, 1, 1), (3, 0, 0), (0, 3, 0), (0, 0, 3), (2, 1, 0), (2, 0, 1),
                (1, 2, 0), (0, 2, 1), (1, 0, 2), (0, 1, 2), (1, 1, 1), (4, 0, 0), (0, 4, 0)]
    k = 0
    while len(species) < nspecies:
        c = clusters[k]
        species.append(''.join(f'{e}{n if n > 1 else ""}' for e, n in zip(new, c) if n))
        rows.append([0] * len(ELEMENTS) + list(c))
        natoms = sum(c)
        # monomers at h = 0; a cluster of n atoms is bound by 20 kJ/mol per extra atom
        h.append(-20e3 * (natoms - 1))
        s.append(150.0 + 30.0 * (natoms - 1) + 2.0 * k)
        k += 1
    h, s = np.array(h, float), np.array(s, float)
    return ch.ChemNetwork(species, elements, rows, TABLE_T, gibbs(TABLE_T, h, s), dex)


def chem_atmosphere(pa, net, L=5, hybrid=True, free_scalars=()):
    """An isothermal WalkerAtmosphere on the 16-species network with [M/H] and C/O free (and a
    hybrid log_H2O), and the parameter vector of its base model."""
    pressure = np.logspace(-6, 1, L)
    models = [pa.MetalEquil(), pa.RatioEquil('C/O')]
    base = [1500.0, 0.0, 0.55]
    if hybrid:
        models.append(pa.IsoVMR('H2O', pressure))
        base.append(-3.5)
    names = ['T_iso'] + [n for m in models for n in m.pnames]
    scalars = {'rplanet': 7.0e9, 'mplanet': 1.5e30, 'log_refpressure': -1.0}
    base += [scalars[s] for s in free_scalars]
    atm = pa.WalkerAtmosphere(pressure, SPECIES, MASS, None, None, pa.Isothermal(pressure),
                              models, rmodel='hydro_m', mplanet=1.5e30, rplanet=7.0e9,
                              refpressure=0.1, free=names + list(free_scalars),
                              base_params=base, chemistry=net)
    return atm, np.array(base)


def element_error(net, vmr, b):
    """Relative error of the result's element ratios against b, per cell: both normalised to
    their hydrogen (b_H = 1)."""
    got = np.asarray(vmr) @ net.stoich.astype(float)
    got = got / got[..., [net.ihydrogen]]
    want = np.asarray(b) / np.asarray(b)[..., [net.ihydrogen]]
    return np.max(np.abs(got / want - 1.0), axis=-1)


def mass_action_residual(net, vmr, temp, pressure):
    """max_i |mu_i - (a pi)_i| of one cell, pi the least-squares fit of mu on a: zero exactly when
    the chemical potentials lie in the span of the stoichiometry, the optimality condition of the
    Gibbs minimum.  mu_i = g_i + ln x_i + ln p."""
    a = net.stoich.astype(float)
    mu = net.gibbs_at([temp])[0] + np.log(vmr) + np.log(pressure)
    pi = np.linalg.lstsq(a, mu, rcond=None)[0]
    return np.max(np.abs(mu - a @ pi))
