"""plan_interp (csrc/pb_interp.hip) through pb_interp_ec_batch_plan: which kernel a batched
interpolation runs, in how many chunks and workgroups, as a table over the shape.  The expected
values are the launch rules stated on their own:

  * walkers per chunk: 64 (or PB_INTERP_CHUNK), halved while ceil(W / 256) * L * ceil(nw / chunk)
    is below 2048 workgroups;
  * two samples per thread when W >= 4, L * W is even and both bases are on 16 bytes -- and only
    without a continuum, which keeps one sample per thread and ceil(W / 256) workgroups in x;
  * two pair slots per thread for up to four species when ceil((W // 2 + 2) / 512) * L * chunks
    still reaches 4096 workgroups; grid.x = ceil((W // 2 + 2) / (256 * slots));
  * species in registers: 4 up to four species, else 8; the unpredicated loop at exactly 4 or 8.

The PB_INTERP_* variables are read at every call.  No GPU needed: the export touches no device."""
import ctypes as C

import pytest

VARS = ('PB_INTERP_CHUNK', 'PB_INTERP_PAIRS', 'PB_INTERP_NP', 'PB_INTERP_FULL')


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


def plan(nmol, L, W, nw, aligned=True, kcont=0, kalk=False):
    from pyratbay_amd import _capi
    out = (C.c_int32 * 6)()
    _capi.call('pb_interp_ec_batch_plan', out, nmol, L, W, nw, int(aligned), kcont, int(kalk))
    return dict(zip(('chunk', 'pairs', 'slots', 'kS', 'kFull', 'gx'), out))


@pytest.mark.parametrize('nmol,L,W,nw,aligned,kcont,chunk,pairs,slots,gx', [
    (4, 32, 770, 64, True, 0, 4, 1, 1, 2),
    (4, 31, 770, 64, True, 0, 2, 1, 1, 2),
    (4, 32, 770, 64, True, 1, 4, None, None, 4),
    (4, 32, 770, 64, False, 0, 4, 0, 1, 4),
    (4, 9, 1501, 37, True, 0, 1, 0, 1, 6),
    (4, 8, 1501, 37, True, 0, 1, 1, 1, 3),
    (1, 128, 31742, 2, True, 0, 64, 1, 2, 32),
    (1, 128, 31738, 2, True, 0, 64, 1, 1, 62),
])
def test_seams(nmol, L, W, nw, aligned, kcont, chunk, pairs, slots, gx):
    p = plan(nmol, L, W, nw, aligned, kcont)
    assert p['chunk'] == chunk and p['gx'] == gx, p
    if pairs is not None:
        assert p['pairs'] == pairs and p['slots'] == slots, p


def test_continuum_forms_keep_one_sample_per_thread():
    for kcont, kalk in ((1, False), (1, True), (2, False), (2, True)):
        assert plan(4, 32, 770, 64, True, kcont, kalk)['gx'] == 4


def test_smallest_grids_with_and_without_pairs():
    assert plan(4, 8, 3, 5)['pairs'] == 0
    assert plan(4, 8, 5, 5)['pairs'] == 1
    assert plan(4, 9, 5, 5)['pairs'] == 0           # L * W odd


@pytest.mark.parametrize('nmol,ks,kfull', [(1, 4, 0), (3, 4, 0), (4, 4, 1), (5, 8, 0), (8, 8, 1)])
def test_species_instantiation(nmol, ks, kfull):
    p = plan(nmol, 8, 1500, 5)
    assert (p['kS'], p['kFull']) == (ks, kfull)


def test_switches_are_read_at_every_call(monkeypatch):
    """The first call of the process (of this test at the latest) has the variables unset; the
    second obeys them: PB_INTERP_FULL and PB_INTERP_PAIRS used to be latched at the first call."""
    p = plan(4, 8, 1500, 5)
    assert (p['kS'], p['kFull'], p['pairs']) == (4, 1, 1)
    monkeypatch.setenv('PB_INTERP_FULL', '0')
    p = plan(4, 8, 1500, 5)
    assert (p['kS'], p['kFull'], p['pairs']) == (4, 0, 1)
    assert plan(8, 8, 1500, 5)['kFull'] == 1        # (the switch is about four species only)
    monkeypatch.delenv('PB_INTERP_FULL')
    monkeypatch.setenv('PB_INTERP_PAIRS', '0')
    p = plan(4, 8, 1500, 5)
    assert (p['kFull'], p['pairs'], p['gx']) == (1, 0, 6)
    monkeypatch.delenv('PB_INTERP_PAIRS')
    p = plan(4, 8, 1500, 5)
    assert (p['kFull'], p['pairs'], p['gx']) == (1, 1, 3)


def test_forced_slots_and_chunk(monkeypatch):
    assert plan(4, 8, 1501, 37)['slots'] == 1
    monkeypatch.setenv('PB_INTERP_NP', '2')
    p = plan(4, 8, 1501, 37)
    assert (p['pairs'], p['slots'], p['gx']) == (1, 2, 2)
    assert plan(8, 8, 1501, 37)['slots'] == 2       # (overrides whatever the species count)
    monkeypatch.setenv('PB_INTERP_NP', '1')
    p = plan(1, 128, 31742, 2)
    assert (p['slots'], p['gx']) == (1, 63)         # ceil((31742 // 2 + 2) / 256)
    monkeypatch.delenv('PB_INTERP_NP')
    # obeyed where the launch is large enough, halved by the workgroup rule where it is not
    monkeypatch.setenv('PB_INTERP_CHUNK', '8')
    assert plan(1, 128, 31742, 2)['chunk'] == 8
    assert plan(4, 32, 770, 64)['chunk'] == 4
    assert plan(4, 9, 1501, 37)['chunk'] == 1


def test_bad_shapes_are_refused():
    from pyratbay_amd import _capi
    for args in ((0, 8, 100, 4, 1, 0, 0), (9, 8, 100, 4, 1, 0, 0), (4, 0, 100, 4, 1, 0, 0),
                 (4, 8, 100, 4, 1, 3, 0)):
        with pytest.raises(_capi.PbError, match='pb_interp_ec_batch_plan: bad shape'):
            _capi.call('pb_interp_ec_batch_plan', (C.c_int32 * 6)(), *args)


def test_work_doubles():
    from pyratbay_amd import _capi
    lib = _capi.lib()
    for L, nw in ((1, 1), (9, 37), (32, 64), (128, 2), (80, 64), (0, 5)):
        n = L * nw
        got = lib.pb_interp_ec_batch_work_doubles(L, nw)
        assert got == 17 * n + 8
        for nmol in range(1, 9):
            ncoef = 4 if nmol <= 4 else 8
            assert got >= 2 * ncoef * n + (n + 1) // 2          # coef[n][2 ncoef] | tlo[n] int32
    assert lib.pb_interp_ec_batch_work_doubles(-1, 4) == -1
    assert lib.pb_interp_ec_batch_work_doubles(4, -1) == -1
