"""The (layer, group) records of the line-by-line extinction after the record kernel's diet
(csrc/pb_ext_records.hip: the sample index without a division and carried from layer to layer
while the oversampling factor stays, the Doppler column searched from the previous layer's, the
quotients by 1 left out, eight layers per thread).  Needs an MI355X.

A case of 2 isotopes, 6 layers and about 400 lines on a grid of 3001 samples, with the lines
where a wrong last bit or a wrong clip would show: lines on the samples of every layer's dynamic
grid (and 1 ulp beside them), lines within one sample of both ends of the grid (the packed
records keep their windows unclipped), a co-added group of three, a line far below the threshold.
At wnosamp 24 the layers take the factors 2, 2, 2, 3, 12, 24 (three layers that carry the index,
three that form it anew, one whose grid has the output step); at wnosamp 6 the upper layers take
the factor 1.

ec against the oracle at the tolerance and zero-pattern rule of tests/test_gpu_extinction.py;
bit for bit the same ec with one layer per thread (PB_REC_LAYERS=1: nothing is carried) and for
wavenumber shards against the slice of the whole call, in every gather mode.  (Different gather
modes agree to rounding, not bit for bit: they add the terms of a sample in different orders.)"""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
RTOL = 1e-10
NL, NISO, NWAVE = 6, 2, 3001
GATHERS = ('staged', 'global', 'auto')


@pytest.fixture(scope='module')
def eng():
    from pyratbay_amd import engine
    engine.require_gpu()
    return engine


def host(t):
    return t.cpu().numpy()


def make_case(wnosamp):
    from pyratbay_amd import synth
    case = synth.lbl_case(NWAVE, NL, 400, wnosamp=wnosamp, nlor=18, ndop=9, extent=80.0,
                          cutoff=3.0, niso=NISO, seed=11)
    g, ln = case['grid'], case['lines']
    own0, ownstep, onwn = g['own'][0], g['ownstep'], g['onwave']
    extra = []                                           # (wavn, isotope, elow, gf)
    # lines on samples of the layers' dynamic grids, and one ulp on either side
    for f in g['divisors']:
        dwnstep = ownstep * int(f)
        last = (onwn - 1) // int(f)
        for n in (0, 1, 2, 4, 5, 63, 64, 65, 1024, last - 1, last):
            if 0 <= n <= last:
                v = own0 + n * dwnstep
                for w in (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
                    if own0 <= w <= g['own'][-1]:
                        extra.append((w, n % NISO, 900.0, 3e-8))
    # within one fine sample and within one output sample of both ends
    for d in (0.3 * ownstep, 0.6 * g['wnstep']):
        extra.append((own0 + d, 0, 500.0, 1e-7))
        extra.append((g['own'][-1] - d, 1, 500.0, 1e-7))
    # a co-added group of three, and a line far below any threshold
    mid = own0 + 0.37 * (g['own'][-1] - own0)
    extra += [(mid, 0, 100.0, 2e-7), (mid + 1e-8, 0, 3000.0, 5e-8), (mid + 2e-8, 0, 7000.0, 1e-6)]
    extra.append((own0 + 0.61 * (g['own'][-1] - own0), 1, 100.0, 1e-70))
    lwn = np.concatenate([ln['lwn'], [e[0] for e in extra]])
    lid = np.concatenate([ln['lid'], np.array([e[1] for e in extra], np.int32)]).astype(np.int32)
    elow = np.concatenate([ln['elow'], [e[2] for e in extra]])
    gf = np.concatenate([ln['gf'], [e[3] for e in extra]])
    order = np.lexsort((lwn, lid))                       # by isotope, then wavenumber
    case['lines'] = dict(lwn=lwn[order], lid=lid[order], elow=elow[order], gf=gf[order])
    return case


class Plan:
    def __init__(self, eng, orc, wnosamp):
        self.case = case = make_case(wnosamp)
        g, atm, ln, iso, vg = (case[k] for k in ('grid', 'atm', 'lines', 'iso', 'voigt'))
        self.vt = eng.VoigtTable.build(vg['lorentz'], vg['doppler'], vg['size'], g['ownstep'],
                                       wnosamp)
        self.ll = eng.LineList(ln['lwn'], ln['elow'], ln['gf'], ln['lid'], NISO, g['own'])
        self.lbl = eng.LBL(self.vt, self.ll, g['wn'], g['divisors'], atm['mol_radius'],
                           atm['mol_mass'], iso['isoimol'], iso['isomass'], iso['isoratio'],
                           iso['isoiext'], vg['cutoff'], 1e-30, max_layers=NL)
        self.args = (eng.dev(atm['temp']), eng.dev(atm['dens']), eng.dev(iso['isoz']))
        # the reference, once: the oracle on its own table, layer by layer
        profile, size, index = cases.oracle_voigt_table(orc, vg, g['ownstep'])
        self.want = np.zeros((NL, 1, g['nwave']))
        for layer in range(NL):
            orc.extinction(self.want[layer], profile, size, index, vg['lorentz'], vg['doppler'],
                           g['wn'], g['own'], g['divisors'], atm['dens'][layer],
                           atm['mol_radius'], atm['mol_mass'], iso['isoimol'], iso['isomass'],
                           iso['isoratio'], iso['isoz'][:, layer].copy(), iso['isoiext'],
                           ln['lwn'], ln['elow'], ln['gf'], ln['lid'], vg['cutoff'], 1e-30,
                           atm['temp'][layer], 0, 1, 0)
        self.want.setflags(write=False)
        self.base = {}

    def run(self, gather, **kw):
        self.lbl.set_gather_mode(gather)
        return host(self.lbl.extinction(*self.args, **kw))

    def whole(self, gather):
        if gather not in self.base:
            self.base[gather] = self.run(gather)
            self.base[gather].setflags(write=False)
        return self.base[gather]


@pytest.fixture(scope='module', params=[24, 6])
def plan(request, eng, orc):
    return Plan(eng, orc, request.param)


def test_case_holds_what_it_is_for(plan):
    g = plan.case['grid']
    assert g['nwave'] == NWAVE and 380 <= len(plan.case['lines']['lwn']) <= 700
    assert plan.ll.nadd >= 2                                  # the group of three, at least
    plan.whole('staged')
    ofactor, kmax = plan.lbl.last_state(NL, 1)
    print('wnosamp', g['wnosamp'], 'ofactor per layer:', ofactor.tolist())
    pairs = list(zip(ofactor[:-1], ofactor[1:]))
    assert any(a != b for a, b in pairs), 'no two adjacent layers with different factors'
    assert any(a == b for a, b in pairs), 'no two adjacent layers that share a factor'
    if g['wnosamp'] == 24:
        assert ofactor[-1] == 24                              # a layer on the output grid's step
    else:
        assert ofactor[0] == 1                                # a layer on the fine grid itself
    assert np.all(kmax > 0)


@pytest.mark.parametrize('gather', GATHERS)
def test_ec_against_the_oracle(plan, gather):
    got = plan.whole(gather)
    worst = 0.0
    for layer in range(NL):
        assert np.array_equal(got[layer] == 0, plan.want[layer] == 0), layer
        nz = plan.want[layer] != 0
        if nz.any():
            worst = max(worst, np.max(np.abs(got[layer][nz] / plan.want[layer][nz] - 1)))
    print(f'{gather}: max rel err vs oracle = {worst:.2e}')
    np.testing.assert_allclose(got, plan.want, rtol=RTOL)


@pytest.mark.parametrize('gather', GATHERS)
def test_layers_per_thread_keep_every_bit(plan, monkeypatch, gather):
    """eight layers per thread (index, cutoff bounds and Doppler column carried) against one"""
    base = plan.whole(gather)
    monkeypatch.setenv('PB_REC_LAYERS', '1')
    assert np.array_equal(plan.run(gather), base)
    monkeypatch.delenv('PB_REC_LAYERS')
    assert np.array_equal(plan.run(gather), base)


@pytest.mark.parametrize('gather', ('staged', 'global'))
def test_shards_equal_the_slice_of_the_whole_call(plan, gather):
    base = plan.whole(gather)
    bounds = [0, 1, 377, 1024, 2999, NWAVE]
    parts = [plan.run(gather, wbegin=a, wcount=b - a) for a, b in zip(bounds[:-1], bounds[1:])]
    assert np.array_equal(np.concatenate(parts, axis=2), base)
