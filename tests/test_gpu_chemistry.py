"""Equilibrium chemistry on the device: pb_equilibrium_vmr (csrc/pb_chemistry.hip) at its boundary
against the solver-independent optimality conditions and ChemNetwork.equilibrium_host,
WalkerAtmosphere(chemistry=net).evaluate against evaluate_host, and a retrieval on [M/H] and C/O.
Every output buffer is pre-filled with NaN (statuses with a sentinel).

Bounds.  Optimality (element ratios against b, mass-action residual): 1e-11, the CPU test's.
Device against host VMRs: 1e-9 relative wherever the host VMR is >= 1e-250 -- two solutions of one
convex problem, each optimal to 1e-11, so loose enough not to flake and tight enough to catch a
wrong sum.  Status: the host's sign, iteration counts within 2.  Closed form: 1e-12.  Every check
prints its figure before it asserts."""
import numpy as np
import pytest

import chemistry_cases as cc

pytestmark = pytest.mark.gpu
SENTINEL = -77


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def ch():
    from pyratbay_amd import chemistry
    return chemistry


@pytest.fixture(scope='module')
def pa():
    from pyratbay_amd import atmosphere
    return atmosphere


@pytest.fixture(scope='module')
def net(ch):
    return cc.network(ch)


def run_kernel(eng, ch, network, temps, pressure, params=None, guard=0, **columns):
    """pb_equilibrium_vmr on NaN-filled outputs; with guard > 0 the outputs are the middle of
    larger buffers whose margins must come back untouched."""
    import torch
    nw, L = temps.shape
    S = network.nspecies
    flat_v = torch.full((guard + nw * L * S + guard,), float('nan'), dtype=torch.float64,
                        device='cuda')
    flat_s = torch.full((guard + nw * L + guard,), SENTINEL, dtype=torch.int32, device='cuda')
    out = (flat_v[guard:guard + nw * L * S].view(nw, L, S), flat_s[guard:guard + nw * L].view(nw, L))
    ch.equilibrium_vmr(network, eng.dev(temps), eng.dev(pressure),
                       None if params is None else eng.dev(params), out=out, **columns)
    torch.cuda.synchronize()
    if guard:
        margins_v = torch.cat([flat_v[:guard], flat_v[guard + nw * L * S:]])
        margins_s = torch.cat([flat_s[:guard], flat_s[guard + nw * L:]])
        assert bool(torch.isnan(margins_v).all()) and bool((margins_s == SENTINEL).all())
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def compare_with_host(vmr, status, want_vmr, want_status, what):
    assert np.array_equal(np.sign(status), np.sign(want_status)), (what, status, want_status)
    ok = want_status > 0
    assert np.all(np.abs(status[ok] - want_status[ok]) <= 2), (what, status, want_status)
    assert np.array_equal(status[~ok], want_status[~ok]) and np.all(vmr[~ok] == 0)
    seen = want_vmr >= 1e-250
    dev = np.max(np.abs(vmr[seen] / want_vmr[seen] - 1.0)) if np.any(seen & ok[..., None]) else 0.0
    print(f'{what}: device vs host VMR max rel {dev:.2e} (bound 1e-9); iterations device '
          f'{status[ok].min() if ok.any() else 0}-{status[ok].max() if ok.any() else 0}, host '
          f'{want_status[ok].min() if ok.any() else 0}-{want_status[ok].max() if ok.any() else 0}')
    assert dev <= 1e-9, (what, dev)
    assert not np.any(np.isnan(vmr))


# ------------------------------------------------------------------------------ kernel boundary
def test_kernel_boundary(eng, ch, net):
    """nw = 3, L = 4: the four grid pressures, twelve grid temperatures, and per-walker [M/H],
    [N/H] and C/O (the first walker's are the base abundances)."""
    pressure = np.array(cc.GRID_P)
    temps = np.array([[300.0, 600.0, 1000.0, 1500.0],
                      [2500.0, 4000.0, 6000.0, 300.0],
                      [6000.0, 1500.0, 600.0, 2500.0]])
    params = np.array([[0.0, 0.0, cc.B[2] / cc.B[4]],
                       [1.0, -0.5, 0.6],
                       [-1.0, 0.3, 1.2]])
    columns = dict(par_metal=0, scales=[(net.elements.index('N'), 1)],
                   ratios=[(net.elements.index('C'), net.elements.index('O'), 2)])
    vmr, status = run_kernel(eng, ch, net, temps, pressure, params, **columns)
    assert np.all(status > 0), status
    worst_elem = worst_mass = 0.0
    for w in range(3):
        b = net.element_abundances_host(params[w, 0], {'N': params[w, 1]}, {'C/O': params[w, 2]})
        want_vmr, _, want_status = net.equilibrium_host(temps[w], pressure, b)
        compare_with_host(vmr[w], status[w], want_vmr, want_status, f'walker {w}')
        worst_elem = max(worst_elem, cc.element_error(net, vmr[w], b).max())
        worst_mass = max([worst_mass] + [cc.mass_action_residual(net, vmr[w, l], temps[w, l],
                                                                 pressure[l]) for l in range(4)])
    print(f'device optimality: element ratios {worst_elem:.2e}, mass action {worst_mass:.2e} '
          '(bounds 1e-11)')
    assert worst_elem <= 1e-11 and worst_mass <= 1e-11


# --------------------------------------------------------------------------------- edge shapes
def test_two_species_closed_form(eng, ch):
    """S = 2, E = 1: H2 <=> 2 H."""
    hyd = cc.hydrogen_network(ch)
    temps, pressure = np.array([[2000.0, 4000.0]]), np.array([1e-3, 1.0])
    vmr, status = run_kernel(eng, ch, hyd, temps, pressure, guard=16)
    assert np.all(status > 0)
    for l in range(2):
        want = cc.hydrogen_closed_form(temps[0, l], pressure[l])
        dev = abs(vmr[0, l, 1] / want - 1.0)
        print(f'x_H at {temps[0, l]} K: {vmr[0, l, 1]:.16e} vs {want:.16e}, rel {dev:.2e}')
        assert dev <= 1e-12 and abs(vmr[0, l, 0] / (1.0 - want) - 1.0) <= 1e-12


def test_largest_network(eng, ch):
    """S = 32 (the most the class accepts), E = 8: the last lanes and the widest system."""
    big = cc.padded_network(ch, 32)
    assert (big.nspecies, big.nelements) == (32, 8)
    b = 10.0**(big.base_dex - 12.0)
    temps = np.array([[300.0, 1000.0, 4000.0], [6000.0, 1500.0, 600.0]])
    pressure = np.array([1e-8, 1e-4, 100.0])
    vmr, status = run_kernel(eng, ch, big, temps, pressure, guard=64)
    for w in range(2):
        want_vmr, _, want_status = big.equilibrium_host(temps[w], pressure, b)
        assert np.all(want_status > 0)
        compare_with_host(vmr[w], status[w], want_vmr, want_status, f'S = 32, walker {w}')
        assert np.all(vmr[w, :, 16:] > 0)


def test_partial_block_and_rejected_walker(eng, ch, net):
    """nw * L = 9 cells (two full blocks of four and one cell); the middle walker has temps = 0 and
    writes zeros and PB_CHEM_REJECTED; its neighbours have the bits of a batch of their own, and
    nothing is written past either end."""
    pressure = np.array([1e-4, 1.0, 100.0])
    temps = np.array([[1000.0, 1500.0, 2500.0], [0.0, 0.0, 0.0], [600.0, 4000.0, 300.0]])
    vmr, status = run_kernel(eng, ch, net, temps, pressure, guard=64)
    assert np.all(vmr[1] == 0) and np.all(status[1] == ch.STATUS_REJECTED)
    for w in (0, 2):
        alone_vmr, alone_status = run_kernel(eng, ch, net, temps[w:w + 1], pressure, guard=64)
        assert np.array_equal(vmr[w], alone_vmr[0]) and np.array_equal(status[w], alone_status[0])
        want_vmr, _, want_status = net.equilibrium_host(temps[w], pressure, cc.B)
        compare_with_host(vmr[w], status[w], want_vmr, want_status, f'walker {w}')
    # every other status path in one batch: outside the table (both ends), NaN, a ratio <= 0
    temps = np.array([[100.0, 7000.0, float('nan')], [1000.0, -3.0, 1000.0]])
    params = np.array([[0.5], [-0.2]])
    ratios = [(net.elements.index('C'), net.elements.index('O'), 0)]
    vmr, status = run_kernel(eng, ch, net, temps, pressure, params, ratios=ratios, guard=64)
    assert status.tolist() == [[ch.STATUS_TEMPERATURE, ch.STATUS_TEMPERATURE, ch.STATUS_REJECTED],
                               [ch.STATUS_RATIO, ch.STATUS_REJECTED, ch.STATUS_RATIO]]
    assert np.all(vmr == 0)


# ---------------------------------------------------------------------------- through the class
def test_evaluate_vs_host(eng, pa, ch, net):
    """nw = 4, L = 5 with [M/H], C/O and a hybrid log_H2O free (and rplanet): temperatures bit for
    bit; densities, mean mass and radius to the free-VMR path's 1e-14 (test_gpu_atmosphere)
    loosened by the 1e-9 of the VMRs; reject bits exactly -- walker 2 leaves the Gibbs table,
    walker 3 has C/O < 0; a second call with out= allocates nothing."""
    import torch
    atm, base = cc.chem_atmosphere(pa, net, L=5, free_scalars=('rplanet',))
    atm.bind(['H2O', 'CO', 'CH4'])
    params = np.stack([base, base + [300.0, 0.7, 0.6, 3.0, 2e8], base + [5400.0, 0, 0, 0, 0],
                       base + [0, 0, -1.0, 0, 0]])
    params_d = eng.dev(params)
    prof = atm.evaluate(params_d)
    torch.cuda.synchronize()
    got = type(prof)(*[None if t is None else t.cpu().numpy() for t in prof])
    tol = 1e-9 + 1e-14
    want_reject = [0, 0, pa.REJECT_CHEMISTRY, pa.REJECT_CHEMISTRY]
    for w in range(4):
        want = atm.evaluate_host(params[w])
        assert want.reject == want_reject[w]
        assert got.reject[w] == want.reject, (w, got.reject[w], want.reject)
        assert np.array_equal(got.temps[w], want.temps)
        if want.reject:
            assert np.all(got.dens[w] == 0) and np.all(got.mm[w] == 0)
            assert np.array_equal(got.radius[w], atm.base_radius)
            continue
        for name in ('dens', 'mm', 'radius'):
            dev = np.max(np.abs(getattr(got, name)[w] / getattr(want, name) - 1.0))
            print(f'walker {w}: {name} vs host max rel {dev:.2e} (tolerance {tol:.0e})')
            assert dev <= tol, (w, name, dev)
    # walker 1's log_H2O = -0.5 is above the cap: its column is the cap (and it is not rejected)
    assert np.all(atm._chain(params[1])['vmr'][:, atm.species.index('H2O')] < 0.01)

    for t in prof:
        if t is not None:
            t.fill_(float('nan') if t.dtype == torch.float64 else SENTINEL)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = atm.evaluate(params_d, out=prof)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert again is prof
    for a, b in zip(again, got):
        assert a is None or np.array_equal(a.cpu().numpy(), b)


def test_out_is_reused_with_chemistry(eng, pa, net):
    """The buffers between the three launches are kept per nw.  nw = 3, L = 5 (walker 2 rejected
    for C/O < 0): a second evaluate(params, out=first) returns the same tensors with the same
    bits, through the same intermediate storage; a call at nw = 5 then gets buffers of its own
    and leaves the nw = 3 result and buffers as they were."""
    import torch
    atm, base = cc.chem_atmosphere(pa, net, L=5, free_scalars=('rplanet',))
    atm.bind(['H2O', 'CO', 'CH4'])
    params = np.stack([base, base + [300.0, 0.7, 0.6, 3.0, 2e8], base + [0, 0, -1.0, 0, 0]])
    params_d = eng.dev(params)
    between = ('temps', 'vmr', 'status')

    def snapshot(nw):
        torch.cuda.synchronize()
        launch = atm.equilibrium_launch(nw, params_d.device)
        return ({k: launch[k].data_ptr() for k in between},
                {k: launch[k].cpu().numpy() for k in between})
    first = atm.evaluate(params_d)
    tensors = tuple(first)
    ptrs, held = snapshot(3)
    want = [None if t is None else t.cpu().numpy() for t in first]
    assert want[-1].tolist() == [0, 0, pa.REJECT_CHEMISTRY]
    assert held['vmr'].shape == (3, 5, net.nspecies) and np.all(held['status'][:2] > 0)

    again = atm.evaluate(params_d, out=first)
    assert again is first and all(a is b for a, b in zip(again, tensors))
    ptrs_again, held_again = snapshot(3)
    assert ptrs_again == ptrs
    for a, b in zip(again, want):
        assert a is None or np.array_equal(a.cpu().numpy(), b)
    for k in between:
        assert np.array_equal(held_again[k], held[k], equal_nan=True)

    more = np.concatenate([params[::-1], params[:2] + [50.0, 0.1, 0.05, 0.2, 1e7]])
    other = atm.evaluate(eng.dev(more))
    ptrs_other, held_other = snapshot(5)
    assert held_other['vmr'].shape == (5, 5, net.nspecies)
    assert not set(ptrs_other.values()) & set(ptrs.values())
    assert other.reject.cpu().numpy()[0] == pa.REJECT_CHEMISTRY
    assert snapshot(3)[0] == ptrs
    for a, b in zip(first, want):
        assert a is None or np.array_equal(a.cpu().numpy(), b)
    for k in between:
        assert np.array_equal(snapshot(3)[1][k], held[k], equal_nan=True)


# ------------------------------------------------------------------------------ through Retrieval
BLOCK = """
    T_iso       1400.0   500.0  3000.0   50.0
    [M/H]          0.0    -2.0     2.0    0.3    0.0    0.5
    C/O           0.55    0.05     2.0    0.1
"""
HYBRID_BLOCK = """
    T_iso       1400.0   500.0  3000.0   50.0
    [M/H]          0.0    -2.0     2.0    0.3
    [C/H]          0.1    -2.0     2.0    0.0
    C/O           0.55    0.05     2.0    0.1
    log_H2O       -3.5    -9.0    -1.0    0.2
"""


def test_retrieval_on_metallicity_and_c_to_o(eng, pa, ch, net, golden):
    """[M/H], C/O and T_iso in a retrieval_params block on the table spectrum of the retrieval
    tests (L = 12, 1000 samples, transit): log_posterior(theta) against evaluate_host's profiles
    fed to eval_bands, the likelihood and log_prior_host.

    Tolerance: the existing end-to-end test allows one rounding of the sum likelihood + prior
    (EPS |total|) between device values.  Here the two sides' VMRs may differ by the 1e-9 above,
    which the densities carry linearly and the mean mass passes to the scale height, so a band
    depth may differ by that times a factor of order one; with ten for that factor, the likelihood
    -0.5 sum ((d - m) / s)^2 may differ by sum |d - m| / s^2 * 1e-8 m."""
    import torch
    import test_gpu_batch_continuum as base
    s = base.setup(golden('g7_continuum'), 4, seed=77, hminus=False, clouds=False)
    wn, pressure = s['wn'], s['pressure']
    L = len(pressure)
    assert (L, len(wn)) == (12, 1000)
    tmodel = pa.Isothermal(pressure)
    common = dict(mplanet=1.2e30, rplanet=7.5e9, refpressure=0.1, chemistry=net)
    atm = pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel,
                              [pa.MetalEquil(), pa.RatioEquil('C/O')],
                              base_params=[1400.0, 0.0, 0.55], **common)
    atm.bind(['H2O', 'CO', 'CH4'])
    model = eng.TableSpectrum(s['etable'], s['ttable'], wn, atm.base_radius, 8.8e10,
                              rt_path='transit', column_order=None)
    _, pb = base.make_bands(eng, wn)
    flux = model.eval_params(atm, eng.dev(atm.base_params[None, :]), pb).cpu().numpy()[0]
    assert np.all(np.isfinite(flux)) and np.all(flux > 0)
    data = flux * (1 + np.random.default_rng(11).normal(0, 0.02, 3))
    uncert = 0.03 * flux
    obs = eng.Observation(data, uncert)
    ret = eng.Retrieval(model, atm, pb, obs, BLOCK)
    assert ret.destination == [('params', 0), ('params', 1), ('params', 2)]

    theta = np.array([[1400.0, 0.0, 0.55], [1650.0, 0.8, 0.9], [1100.0, -0.6, 0.3],
                      [1500.0, 0.2, 1.1]])
    assert np.all(ret.inside_host(theta))
    post = ret.log_posterior(eng.dev(theta))
    torch.cuda.synchronize()
    post = post.cpu().numpy()
    params = ret.split_host(theta)['params']
    profs = [atm.evaluate_host(p) for p in params]
    assert all(p.reject == 0 for p in profs)
    host_flux = model.eval_bands(eng.dev(np.stack([p.temps for p in profs])),
                                 eng.dev(np.stack([p.dens for p in profs])), pb,
                                 radius=eng.dev(np.stack([p.radius for p in profs])))
    want_like = obs.loglike(host_flux).cpu().numpy()
    host_flux = host_flux.cpu().numpy()
    want = want_like + ret.log_prior_host(theta)
    eps = np.finfo(float).eps
    bound = eps * np.abs(want) + \
        np.sum(np.abs(data - host_flux) / uncert**2 * 1e-8 * host_flux, axis=1)
    print('log-posterior device', post, 'host profiles', want, 'difference', post - want,
          'bound', bound)
    assert np.all(np.isfinite(post)) and np.all(post > -1e6)
    assert np.all(np.abs(post - want) <= bound)
    assert len(set(np.round(post, 6))) == 4             # [M/H] and C/O move the spectrum

    # the reference's other names resolve as well, each to its column
    hybrid = pa.WalkerAtmosphere(pressure, cc.SPECIES, cc.MASS, None, None, tmodel,
                                 [pa.MetalEquil(), pa.ScaleEquil('[C/H]'), pa.RatioEquil('C/O'),
                                  pa.IsoVMR('H2O', pressure)],
                                 base_params=[1400.0, 0.0, 0.1, 0.55, -3.5], **common)
    hybrid.bind(['H2O', 'CO', 'CH4'])
    ret = eng.Retrieval(model, hybrid, pb, obs, HYBRID_BLOCK)
    assert ret.pnames == ['T_iso', '[M/H]', '[C/H]', 'C/O', 'log_H2O']
    assert ret.destination == [('params', k) for k in range(5)]
    like = ret.log_likelihood(eng.dev(np.array([[1400.0, 0.0, 0.55, -3.5]])))
    assert bool(torch.isfinite(like).all()) and float(like[0]) > -1e6
