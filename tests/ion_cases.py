"""Shared cases of the tests of equilibrium chemistry with ions and electrons (CPU and GPU): a
14-species H-He-O-Na-K network with H+, H-, e-, Na+ and K+ on the synthetic Gibbs recipe of
chemistry_cases.py, the Saha network H, H+, e-, the 16-species network with ions added, a
32-species network of 7 elements and the charge balance, and the optimality measures on
net.balance = [stoich | charges]."""
import numpy as np

import chemistry_cases as cc

ELECTRON_MASS = 5.48579909e-4
SPECIES = ['H2', 'H', 'He', 'H2O', 'OH', 'O', 'O2', 'Na', 'K', 'H+', 'H-', 'e-', 'Na+', 'K+']
ELEMENTS = ['H', 'He', 'O', 'Na', 'K']
STOICH = np.array([
    # H He  O Na  K
    [2, 0, 0, 0, 0],    # H2
    [1, 0, 0, 0, 0],    # H
    [0, 1, 0, 0, 0],    # He
    [2, 0, 1, 0, 0],    # H2O
    [1, 0, 1, 0, 0],    # OH
    [0, 0, 1, 0, 0],    # O
    [0, 0, 2, 0, 0],    # O2
    [0, 0, 0, 1, 0],    # Na
    [0, 0, 0, 0, 1],    # K
    [1, 0, 0, 0, 0],    # H+
    [1, 0, 0, 0, 0],    # H-
    [0, 0, 0, 0, 0],    # e-
    [0, 0, 0, 1, 0],    # Na+
    [0, 0, 0, 0, 1],    # K+
])
CHARGES = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, -1, -1, 1, 1])
CATIONS = [9, 12, 13]
MASS = np.array([2.01588, 1.00794, 4.002602, 18.01528, 17.00734, 15.9994, 31.9988, 22.98977,
                 39.0983, 1.00739, 1.00849, ELECTRON_MASS, 22.98922, 39.09775])
# g_i(T) = (h_i - T s_i) / (8.314 T): the neutrals of chemistry_cases.py, Na and K vapour, and the
# ions at 1536, 139, 0, 609 and 514 kJ/mol
H_FORM = np.array([0, 218, 0, -242, 39, 249, 0, 107, 89, 1536, 139, 0, 609, 514]) * 1e3
S_ENT = np.array([130, 115, 126, 189, 184, 161, 205, 154, 160, 109, 109, 21, 148, 154.0])
B = np.array([1.0, 0.085, 4.9e-4, 1.7e-6, 1.2e-7])          # H, He, O, Na, K
BASE_DEX = 12.0 + np.log10(B)


def network(ch, cation_enthalpy=None, charges=CHARGES):
    """The 14-species network of the module docstring; cation_enthalpy (J/mol): the enthalpy of
    H+, Na+ and K+ alike, in place of their own."""
    h = H_FORM.astype(float)
    if cation_enthalpy is not None:
        h[CATIONS] = cation_enthalpy
    return ch.ChemNetwork(SPECIES, ELEMENTS, STOICH, cc.TABLE_T, cc.gibbs(cc.TABLE_T, h, S_ENT),
                          BASE_DEX, charges=charges)


def neutral_subnetwork(ch):
    """The nine neutral species of the 14 alone, a network without charges."""
    keep = CHARGES == 0
    return ch.ChemNetwork([s for s, k in zip(SPECIES, keep) if k], ELEMENTS, STOICH[keep],
                          cc.TABLE_T, cc.gibbs(cc.TABLE_T, H_FORM[keep], S_ENT[keep]), BASE_DEX)


def saha_network(ch):
    """H <=> H+ + e- (S = 3, E = 1)."""
    h, s = H_FORM[[1, 9, 11]], S_ENT[[1, 9, 11]]
    return ch.ChemNetwork(['H', 'H+', 'e-'], ['H'], [[1], [1], [0]], cc.TABLE_T,
                          cc.gibbs(cc.TABLE_T, h, s), [12.0], charges=[0, 1, -1])


def saha_closed_form(temp, pressure):
    """x_H+ = x_e = alpha / (1 + alpha), alpha = sqrt(K / (K + p)), K = exp(g_H - g_H+ - g_e)."""
    g = cc.gibbs([temp], H_FORM[[1, 9, 11]], S_ENT[[1, 9, 11]])[0]
    K = np.exp(g[0] - g[1] - g[2])
    alpha = np.sqrt(K / (K + pressure))
    return alpha / (1.0 + alpha)


ION_NAMES = ['H+', 'H-', 'e-', 'Na', 'Na+', 'K', 'K+']


def sixteen_with_ions(ch):
    """The 16-species network of chemistry_cases.py with H+, H-, e-, Na, Na+, K and K+ added (23
    species, 7 elements) -> the network, its molar masses and its b."""
    pick = [SPECIES.index(s) for s in ION_NAMES]
    species = list(cc.SPECIES) + ION_NAMES
    elements = list(cc.ELEMENTS) + ['Na', 'K']
    rows = [list(r) + [0, 0] for r in cc.STOICH]
    for i in pick:
        rows.append([int(STOICH[i, 0]), 0, 0, 0, 0, int(STOICH[i, 3]), int(STOICH[i, 4])])
    h = np.concatenate([cc.H_FORM, H_FORM[pick]]).astype(float)
    s = np.concatenate([cc.S_ENT, S_ENT[pick]])
    charges = np.concatenate([np.zeros(16, int), CHARGES[pick]])
    dex = list(cc.BASE_DEX) + list(BASE_DEX[3:])
    mass = np.concatenate([cc.MASS, MASS[pick]])
    net = ch.ChemNetwork(species, elements, rows, cc.TABLE_T, cc.gibbs(cc.TABLE_T, h, s), dex,
                         charges=charges)
    return net, mass, np.concatenate([cc.B, B[3:]])


def sixteen_with_trace_ions(ch, cation_enthalpy=670e3):
    """The 16-species network with H+, H- and e- alone added (no new element): with H+ at 670
    kJ/mol the ions are about 1e-16 of the gas at 1000 K and 1 bar, inert traces."""
    pick = [SPECIES.index(s) for s in ('H+', 'H-', 'e-')]
    h = np.concatenate([cc.H_FORM, H_FORM[pick]]).astype(float)
    h[16] = cation_enthalpy
    s = np.concatenate([cc.S_ENT, S_ENT[pick]])
    rows = [list(r) for r in cc.STOICH] + [[1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    return ch.ChemNetwork(list(cc.SPECIES) + ['H+', 'H-', 'e-'], cc.ELEMENTS, rows, cc.TABLE_T,
                          cc.gibbs(cc.TABLE_T, h, s), cc.BASE_DEX,
                          charges=[0] * 16 + [1, -1, -1])


def padded_network(ch, nspecies=32):
    """sixteen_with_ions padded like chemistry_cases.padded_network: 7 elements and the charge
    balance (the matrix of the neutral E = 8), then inert clusters of Na and K up to nspecies."""
    net, _, b = sixteen_with_ions(ch)
    species, rows = list(net.species), [list(r) for r in net.stoich]
    h = list(np.concatenate([cc.H_FORM, H_FORM[[SPECIES.index(s) for s in ION_NAMES]]]))
    s = list(np.concatenate([cc.S_ENT, S_ENT[[SPECIES.index(s) for s in ION_NAMES]]]))
    charges = list(net.charges)
    clusters = [(2, 0), (0, 2), (1, 1), (3, 0), (0, 3), (2, 1), (1, 2), (4, 0), (0, 4)]
    k = 0
    while len(species) < nspecies:
        c = clusters[k]
        species.append(''.join(f'{e}{n if n > 1 else ""}' for e, n in zip(('Na', 'K'), c) if n))
        rows.append([0] * 5 + list(c))
        natoms = sum(c)
        h.append(100e3 * natoms - 20e3 * (natoms - 1))
        s.append(150.0 + 30.0 * (natoms - 1) + 2.0 * k)
        charges.append(0)
        k += 1
    padded = ch.ChemNetwork(species, net.elements, rows, cc.TABLE_T,
                            cc.gibbs(cc.TABLE_T, np.array(h, float), np.array(s, float)),
                            net.base_dex, charges=charges)
    return padded, b


def neutrality(net, vmr):
    """|sum_i q_i x_i| / sum_i |q_i| x_i per cell (0 where no ion has a density)."""
    q = net.charges.astype(float)
    vmr = np.asarray(vmr, float)
    total = vmr @ np.abs(q)
    with np.errstate(all='ignore'):
        return np.where(total > 0.0, np.abs(vmr @ q) / total, 0.0)


def element_error(net, vmr, b):
    """chemistry_cases.element_error (net.stoich holds no charge)."""
    return cc.element_error(net, vmr, b)


def mass_action_residual(net, vmr, temp, pressure):
    """chemistry_cases.mass_action_residual on net.balance, over the species with a density: the
    potentials of a minimum lie in the span of [stoich | charges]."""
    a = net.balance.astype(float)
    vmr = np.asarray(vmr, float)
    has = vmr > 0.0
    mu = net.gibbs_at([temp])[0][has] + np.log(vmr[has]) + np.log(pressure)
    pi = np.linalg.lstsq(a[has], mu, rcond=None)[0]
    return np.max(np.abs(mu - a[has] @ pi))
