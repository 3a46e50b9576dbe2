"""Atmospheres from retrieval parameters on the device: WalkerAtmosphere.evaluate
(pb_walker_atmosphere, csrc/pb_atmosphere.hip) against fixture G22 and the host forms, its reject
contract, TableSpectrum.eval_params against eval_bands, and graph capture.

Tolerances: the worst relative deviation measured on one MI355X over every case of this file,
times ten, rounded up to a power of ten; a measured 0 stays "equal bits".  Every check prints its
figure before it asserts.  Measured (profiles/atmosphere.md has the same table):
                              vs G22      vs evaluate_host
  temperature, isothermal     0           0
  temperature, guillot        6.7e-16     4.4e-16
  temperature, madhu          0           0
  density (VMR x p / kT)      8.9e-16     8.9e-16
  mean molecular mass         2.2e-16     2.2e-16
  radius, hydro_m             2.2e-16     3.3e-16
  radius, hydro_g             1.1e-16     2.2e-16
The VMR itself is no output of the kernel; the density carries it (times p / kT)."""
import numpy as np
import pytest

import atm_cases as ac

pytestmark = pytest.mark.gpu

# name: (tolerance against G22, tolerance against the host form)
TOL = {
    'temp_isothermal': (0.0, 0.0),
    'temp_guillot': (1e-14, 1e-14),
    'temp_madhu': (0.0, 0.0),
    'dens': (1e-14, 1e-14),
    'mm': (1e-14, 1e-14),
    'radius_hydro_m': (1e-14, 1e-14),
    'radius_hydro_g': (1e-14, 1e-14),
}
G = ac.g22()
CASES = list(enumerate(G['case_list']))
IDS = [f'c{i}-{c["group"]}' for i, c in CASES]


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope='module')
def pa():
    from pyratbay_amd import atmosphere
    return atmosphere


def host(t):
    return None if t is None else t.cpu().numpy()


def check(name, which, got, want, what):
    dev = ac.max_rel(got, want)
    tol = TOL[name][which]
    print(f'{what}: {name} vs {("G22", "host")[which]} max rel {dev:.2e} (tolerance {tol:.0e})')
    assert dev <= tol, (what, name, dev)


def assert_rejected(pa, prof, w, bit, atm, ntab=4):
    assert prof.reject[w] & bit, (w, prof.reject[w], bit)
    assert np.all(prof.temps[w] == 0) and np.all(prof.dens[w] == 0) and np.all(prof.mm[w] == 0)
    assert prof.dens[w].shape == (atm.nlayers, ntab)
    assert np.array_equal(prof.radius[w], atm.base_radius)


def run(eng, atm, params):
    import torch
    prof = atm.evaluate(eng.dev(np.atleast_2d(params)))
    torch.cuda.synchronize()
    return type(prof)(*[host(t) for t in prof])


@pytest.mark.parametrize('i,case', CASES, ids=IDS)
def test_evaluate_vs_g22(eng, pa, i, case):
    """Every case of G22 (the reference's own functions chained in calc_profiles' order), per
    output.  The three cases the reference computes but the device rejects -- madhu with
    log_p1 > log_p3 (the reference's temperatures are 0 too), the trace abundances above qcap, the
    divergent hydro_m profile -- must come out with their bit and the reject contract.
    Measured worst deviations: isothermal and madhu temperatures 0, guillot 6.7e-16, density
    8.9e-16, mean mass 2.2e-16, radius hydro_m 2.2e-16, hydro_g 1.1e-16; tolerances 0 and 1e-14."""
    atm, params = ac.walker_atmosphere(case)
    prof = run(eng, atm, np.stack([params, params]))
    for out in prof:
        assert out is None or np.array_equal(out[0], out[1])
    itab = [atm.species.index(s) for s in ac.TABLE_SPECIES]
    if case['stops_after'] == 'temp':
        assert np.all(G[f'c{i}_temp'] == 0)
        assert_rejected(pa, prof, 0, pa.REJECT_MADHU, atm)
        assert prof.reject[0] == pa.REJECT_MADHU | pa.REJECT_TEMP
        return
    if case['qcap_flag'] or case['divergent']:
        bit = pa.REJECT_QCAP if case['qcap_flag'] else pa.REJECT_DIVERGENT
        assert_rejected(pa, prof, 0, bit, atm)
        assert prof.reject[0] == bit
        return
    assert prof.reject[0] == 0
    what = f'case {i} ({case["group"]}, {case["grid"]})'
    check('temp_' + case['tmodel'], 0, prof.temps[0], G[f'c{i}_temp'], what)
    check('dens', 0, prof.dens[0], G[f'c{i}_dens'][:, itab], what)
    check('mm', 0, prof.mm[0], G[f'c{i}_mm'], what)
    check('radius_' + case['rmodel'], 0, prof.radius[0], G[f'c{i}_radius'], what)


def random_model(pa, L, nspec, kind, seed):
    """A model of `kind` on L layers with 3 or 6 species and nw parameter vectors around a base."""
    rng = np.random.default_rng(seed)
    pressure = np.logspace(-8, 2, L)
    x = np.linspace(0, 1, L)
    if nspec == 3:
        species, mass, bulk = ['H2', 'He', 'H2O'], [2.01588, 4.002602, 18.01528], ['H2', 'He']
        vmr = np.stack([0.85 - 4e-4 * x, 0.1496 + 0 * x, 4e-4 * (1 + x)], axis=1)
        vmr_models = [pa.IsoVMR('H2O', pressure)]
        vbase, vwidth = [-3.3], [0.5]
        table = ['H2O']
    else:
        species, mass, bulk = [str(s) for s in G['species']], G['mass'], ['H2']
        vmr = np.stack([0.85 + 0 * x, 0.149 * (1 + 0.05 * np.cos(3 * x)), 4e-4 * (1 + 0.5 * x),
                        1e-4 * (1 - 0.3 * x), 5e-4 * (1 + 0.2 * np.sin(5 * x)), 1e-7 + 0 * x],
                       axis=1)
        vmr_models = [pa.SlantVMR('H2O', pressure), pa.ScaleVMR('CH4', pressure, vmr[:, 3]),
                      pa.IsoVMR('CO2', pressure)]
        vbase = [0.5, -3.3, -3.0, -6.0, -2.5, 0.2, -5.5]
        vwidth = [0.3, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
        table = ac.TABLE_SPECIES
    if kind == 'guillot':
        tmodel = pa.Guillot(pressure, 2200.0)
        tbase, twidth = [-1.5, -0.8, 0.2, 0.4, 1400.0, 150.0], [0.5, 0.5, 0.5, 0.3, 300.0, 50.0]
    elif kind == 'madhu':
        tmodel = pa.Madhu(pressure)
        tbase, twidth = [-3.5, -2.0, 0.5, 3.0, 0.6, 1200.0], [0.5, 1.5, 0.4, 0.5, 0.1, 200.0]
    else:
        tmodel = pa.Isothermal(pressure)
        tbase, twidth = [1500.0], [600.0]
    rmodel = 'hydro_g' if kind == 'madhu' else 'hydro_m'
    free = list(tmodel.pnames) + [n for m in vmr_models for n in m.pnames]
    scalars = ['log_refpressure'] if kind == 'madhu' else ['rplanet', 'mplanet']
    sbase = [-1.3] if kind == 'madhu' else [7.1e9, 1.5e30]
    swidth = [1.0] if kind == 'madhu' else [5e8, 4e29]
    atm = pa.WalkerAtmosphere(pressure, species, mass, vmr, bulk, tmodel, vmr_models,
                              rmodel=rmodel, gplanet=2400.0, rplanet=7.0e9, refpressure=0.1,
                              mplanet=1.5e30, base_radius=np.linspace(8e9, 7e9, L),
                              free=free + scalars)
    atm.bind(table)

    def draw(nw):
        base, width = np.array(tbase + vbase + sbase), np.array(twidth + vwidth + swidth)
        return base + width * rng.uniform(-1, 1, (nw, len(base)))
    return atm, draw


@pytest.mark.parametrize('nspec', [3, 6])
@pytest.mark.parametrize('L', [2, 11, 64, 65, 130])
@pytest.mark.parametrize('nw', [1, 3, 65])
def test_evaluate_vs_host(eng, pa, nw, L, nspec):
    """Random parameters, walker by walker against evaluate_host: one walker and more than a
    wavefront's worth of them, layer counts at and across the wavefront (64, 65) and through the
    loop (130), 3 species (one model, two bulk species) and 6 (three models, one bulk species);
    the three T models, both radius models and all three free scalars take turns.
    Measured worst deviations: isothermal and madhu temperatures 0, guillot 4.4e-16, density
    8.9e-16, mean mass 2.2e-16, radius hydro_m 3.3e-16, hydro_g 2.2e-16; tolerances 0 and 1e-14."""
    kind = ('guillot', 'madhu', 'isothermal')[(L + nw + nspec) % 3]
    atm, draw = random_model(pa, L, nspec, kind, seed=1000 * L + 10 * nw + nspec)
    params = draw(nw)
    prof = run(eng, atm, params)
    accepted = 0
    for w in range(nw):
        want = atm.evaluate_host(params[w])
        assert prof.reject[w] == want.reject, (w, prof.reject[w], want.reject)
        if want.reject:
            assert_rejected(pa, prof, w, want.reject, atm, ntab=len(atm._table_species))
            continue
        accepted += 1
        what = f'{kind} L={L} walker {w}'
        check('temp_' + kind, 1, prof.temps[w], want.temps, what)
        check('dens', 1, prof.dens[w], want.dens, what)
        check('mm', 1, prof.mm[w], want.mm, what)
        check('radius_' + atm.rmodel, 1, prof.radius[w], want.radius, what)
    assert accepted >= (nw + 1) // 2


def test_every_reject_reason(eng, pa):
    """Each reason sets its bit and gives temps = 0, zero densities and the base radius; the
    walkers in between come out exactly as they do in a batch of their own."""
    case = dict(G['case_list'][14], qcap=0.2)
    atm, good = ac.walker_atmosphere(case, free_scalars=('log_refpressure', 'mplanet'))
    ilog, imass = atm.npar - 2, atm.npar - 1
    rows, bits = [], []

    def add(bit, **change):
        p = good.copy()
        for k, v in change.items():
            p[int(k[1:])] = v
        rows.append(p)
        bits.append(bit)
    add(0)
    add(pa.REJECT_TEMP, _4=0.0, _5=0.0)                       # T_irr = T_int = 0
    add(0, _6=-3.6)
    add(pa.REJECT_QCAP, _6=-0.5)                              # log H2O: 0.32 > qcap
    add(pa.REJECT_REFPRESSURE, **{f'_{ilog}': 2.5})           # 316 bar: below the last layer
    add(0, **{f'_{ilog}': -2.0})
    add(pa.REJECT_REFPRESSURE, **{f'_{ilog}': float('nan')})
    add(pa.REJECT_DIVERGENT, **{f'_{imass}': 1.0e27})
    add(pa.REJECT_TEMP, _4=float('nan'))
    add(0, **{f'_{imass}': 2.0e30})
    params = np.array(rows)
    prof = run(eng, atm, params)
    assert prof.reject.dtype == np.int32
    keep = [w for w, b in enumerate(bits) if b == 0]
    alone = run(eng, atm, params[keep])
    for w, bit in enumerate(bits):
        if bit:
            # (its own bit; T = 0 everywhere also makes a flat, hence "divergent", radius: the
            # whole mask is the host form's)
            assert prof.reject[w] == atm.evaluate_host(params[w]).reject, (w, prof.reject[w])
            assert_rejected(pa, prof, w, bit, atm)
        else:
            assert prof.reject[w] == 0
            assert np.all(prof.temps[w] > 0) and np.all(prof.dens[w] > 0)
            k = keep.index(w)
            for a, b in zip(prof, alone):
                assert a is None or np.array_equal(a[w], b[k])
    # madhu: log_p1 > log_p3
    matm, mgood = ac.walker_atmosphere(G['case_list'][8])
    bad = mgood.copy()
    bad[0] = 1.0
    mprof = run(eng, matm, np.stack([mgood, bad, mgood]))
    assert list(mprof.reject) == [0, pa.REJECT_MADHU | pa.REJECT_TEMP, 0]
    assert_rejected(pa, mprof, 1, pa.REJECT_MADHU, matm)
    assert np.array_equal(mprof.temps[0], mprof.temps[2]) and np.all(mprof.temps[0] > 0)


@pytest.mark.parametrize('rmodel', ['hydro_m', 'hydro_g'])
def test_bad_free_scalars_are_rejected(eng, pa, rmodel):
    """A free rplanet or mplanet that is NaN, zero or negative gives no geometry: such a walker
    has the divergent bit (every comparison of the decrease rule is false on NaN, so the kernel
    tests the radius itself), the reject contract holds, and the host form gives the same mask."""
    i, case = next((i, c) for i, c in CASES if c['rmodel'] == rmodel and c['group'] == 'radius'
                   and not c['divergent'])
    scalars = ('rplanet', 'mplanet') if rmodel == 'hydro_m' else ('rplanet',)
    atm, good = ac.walker_atmosphere(case, free_scalars=scalars)
    rows = [good.copy()]
    for k in range(len(scalars)):
        for bad in (float('nan'), 0.0, -good[atm.npar - len(scalars) + k], float('inf')):
            p = good.copy()
            p[atm.npar - len(scalars) + k] = bad
            rows.append(p)
    rows.append(good.copy())
    params = np.array(rows)
    prof = run(eng, atm, params)
    for w in (0, len(rows) - 1):
        assert prof.reject[w] == 0 and np.all(np.isfinite(prof.radius[w]))
        assert np.array_equal(prof.radius[w], prof.radius[0])
    for w in range(1, len(rows) - 1):
        assert prof.reject[w] == atm.evaluate_host(params[w]).reject, (w, prof.reject[w])
        assert_rejected(pa, prof, w, pa.REJECT_DIVERGENT, atm)


@pytest.fixture(scope='module')
def g7(golden):
    return golden('g7_continuum')


def spectrum_case(eng, pa, g7, nw, seed, continuum, deck):
    import test_gpu_batch_alkali as alk
    import test_gpu_batch_continuum as base
    from pyratbay_amd import continuum as ct
    s = base.setup(g7, nw, seed=seed, hminus=True, clouds=False)
    wn, pressure = s['wn'], s['pressure']
    L = len(pressure)
    assert (L, len(wn)) == (12, 1000)
    cont = None
    if continuum:
        models = s['models'] + alk.alkali_models(g7, ct, pressure)
        if deck:
            models = models + [ct.Deck(pressure, wn)]
        cont = ct.Continuum(wn, pressure, models)
        assert cont.species == ['H2', 'He', 'H', 'e-'] and cont.alkali_species == ['Na', 'K']
    species = ['H2', 'He', 'H', 'e-', 'Na', 'K', 'H2O', 'CO', 'CH4']
    mass = [2.01588, 4.002602, 1.00794, 5.4858e-4, 22.98977, 39.0983, 18.01528, 28.0101, 16.0425]
    vmr = np.tile([0.85, 0.148, 1e-3, 1e-6, 2e-6, 1.5e-7, 4e-4, 5e-4, 1e-4], (L, 1))
    tmodel = pa.Guillot(pressure, 2200.0)
    vmr_models = [pa.IsoVMR('H2O', pressure), pa.IsoVMR('CO', pressure),
                  pa.ScaleVMR('Na', pressure, vmr[:, 4])]
    free = list(tmodel.pnames) + [n for m in vmr_models for n in m.pnames] + ['rplanet']
    base_params = np.array([-1.5, -0.8, 0.2, 0.4, 1400.0, 150.0, -3.4, -3.3, 0.0, 7.5e9])
    atm = pa.WalkerAtmosphere(pressure, species, mass, vmr, ['H2', 'He'], tmodel, vmr_models,
                              mplanet=1.2e30, refpressure=0.1, qcap=0.1, free=free,
                              base_params=base_params)
    atm.bind(['H2O', 'CO', 'CH4'], cont)
    rng = np.random.default_rng(seed)
    params = base_params * (1 + 0.05 * rng.uniform(-1, 1, (nw, len(base_params))))
    params[1, 4:6] = 0.0                     # rejected: T = 0
    params[nw - 2, 6] = -0.3                 # rejected: above qcap
    s.update(cont=cont, atm=atm, params=params, rejected=[1, nw - 2],
             base_radius=atm.base_radius)
    return s


@pytest.mark.parametrize('rt_path,continuum,deck', [('transit', False, False),
                                                    ('emission', False, False),
                                                    ('transit', True, False),
                                                    ('emission', True, True)])
def test_eval_params_vs_eval_bands(eng, pa, g7, rt_path, continuum, deck):
    """eval_params(...) is eval_bands(...) on the tensors evaluate() returns, bit for bit, and the
    walkers the atmosphere rejects come out as +inf: L = 12, W = 1000, chunks of 4, both
    geometries; once with Rayleigh + CIA + H- + Na/K, where continuum_density and alkali_density
    come through the index maps, and once with a cloud deck at per-walker pressures.  The two
    density outputs against evaluate_host are densities like any other: the density tolerance,
    1e-14 (worst density measured against the host form: 8.9e-16)."""
    import torch
    import test_gpu_batch_continuum as base
    nw = 9
    s = spectrum_case(eng, pa, g7, nw, 77, continuum, deck)
    atm, cont = s['atm'], s['cont']
    model = eng.TableSpectrum(s['etable'], s['ttable'], s['wn'], s['base_radius'], 8.8e10,
                              rt_path=rt_path, continuum=cont)
    _, pb = base.make_bands(eng, s['wn'])
    params = eng.dev(s['params'])
    kw = dict(chunk=4)
    if deck:
        kw['deck_logp'] = eng.dev(np.random.default_rng(5).uniform(-3.0, 0.5, nw))
    got = model.eval_params(atm, params, pb, **kw)
    prof = atm.evaluate(params)
    if continuum:
        assert prof.continuum_density.shape == (nw, 12, 4)
        assert prof.alkali_density.shape == (nw, 12, 2)
        kw.update(continuum_density=prof.continuum_density, alkali_density=prof.alkali_density)
        # through the index maps: the same numbers as the table's columns of the same species
        want = atm.evaluate_host(s['params'][0])
        check('dens', 1, host(prof.continuum_density[0]), want.continuum_density, 'continuum')
        check('dens', 1, host(prof.alkali_density[0]), want.alkali_density, 'alkali')
    else:
        assert prof.continuum_density is None and prof.alkali_density is None
    want = model.eval_bands(prof.temps, prof.dens, pb, radius=prof.radius, **kw)
    torch.cuda.synchronize()
    got, want = host(got), host(want)
    assert np.array_equal(got, want)
    reject = host(prof.reject)
    assert [w for w in range(nw) if reject[w]] == s['rejected']
    for w in range(nw):
        if reject[w]:
            assert np.all(np.isposinf(got[w])), w
        else:
            assert np.all(np.isfinite(got[w])) and np.all(got[w] > 0), w
    with pytest.raises(ValueError, match='comes from the atmosphere'):
        model.eval_params(atm, params, pb, radius=prof.radius)


def capture_or_skip(torch):
    """Whether this build can capture at all is settled on a torch op, before the code under test
    runs: whatever evaluate() raises under capture is then a failure, not a skip."""
    if not hasattr(torch.cuda, 'CUDAGraph') or not hasattr(torch.cuda, 'graph'):
        pytest.skip('graph capture is unavailable: this torch has no torch.cuda.CUDAGraph')
    probe = torch.zeros(8, device='cuda')
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            probe.add_(1.0)
        g.replay()
        torch.cuda.synchronize()
    except (RuntimeError, AttributeError) as exc:        # pragma: no cover
        pytest.skip(f'graph capture is unavailable: a probe capture of one torch op failed: {exc}')
    assert float(probe.sum()) == 8.0


def graph_case(eng, pa):
    import torch
    atm, draw = random_model(pa, 65, 6, 'guillot', seed=9)
    params = eng.dev(draw(5))
    eager = atm.evaluate(params)
    out = atm.evaluate(params)                       # the buffers the graph writes
    for t in out:
        if t is not None:
            t.zero_()
    torch.cuda.synchronize()
    return atm, params, eager, out


def test_graph_capture(eng, pa):
    """evaluate() captured into a graph and replayed gives the tensors of the eager call, bit for
    bit: no allocation, no synchronisation and no read-back inside (any of them raises under
    capture and fails this test)."""
    import torch
    capture_or_skip(torch)
    atm, params, eager, out = graph_case(eng, pa)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        atm.evaluate(params, out=out)
    torch.cuda.synchronize()
    assert not out.temps.any()                       # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert int((eager.reject == 0).sum()) >= 3
    for a, b in zip(eager, out):
        assert a is None or torch.equal(a, b)


def dot_nodes_and_edges(text):
    """(node statements, edge statements) of a Graphviz dump, the defaults `node [`, `edge [` and
    `graph [` and the subgraph braces left out."""
    import re
    nodes, edges = [], []
    for line in text.splitlines():
        line = line.strip()
        if '->' in line:
            edges.append(line)
        elif re.match(r'^"?[\w.:-]+"?\s*\[', line) and \
                not re.match(r'^(node|edge|graph)\s*\[', line):
            nodes.append(line)
    return nodes, edges


def test_graph_is_one_kernel(eng, pa, tmp_path):
    """The captured graph is a single kernel node, k_walker_atmosphere, with no edge: exactly one
    node is counted in the runtime's own dump of the graph, so two independent nodes (a parallel
    branch without an edge) fail as well."""
    import torch
    capture_or_skip(torch)
    if not hasattr(torch.cuda.CUDAGraph, 'debug_dump'):
        pytest.skip('this torch cannot dump a captured graph (no CUDAGraph.debug_dump)')
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)      # the captured graph stays for the dump
    except TypeError:
        graph = torch.cuda.CUDAGraph()
        graph.enable_debug_mode()
    atm, params, eager, out = graph_case(eng, pa)
    with torch.cuda.graph(graph):
        atm.evaluate(params, out=out)
    path = tmp_path / 'graph.dot'
    graph.debug_dump(str(path))
    text = path.read_text() if path.exists() else ''
    if not text.strip():
        pytest.skip('the runtime wrote no dump of the captured graph')
    print(text)
    nodes, edges = dot_nodes_and_edges(text)
    assert edges == [], text
    assert len(nodes) == 1, text
    assert 'k_walker_atmosphere' in text, text
