"""plan_eval_bands (pyratbay_amd/table.py): which kernels the chunks of a TableSpectrum.eval_bands
call run, as a truth table over the plain facts it is given.  The expected values are the rules of
the batch, stated here on their own:

  * two-stream geometry is never ordered (no stop to order the columns for);
  * the one-pass transit only in transit geometry, without a Continuum, and not for a cloudy call;
  * a cloudy call runs in the column order in use but never under its layer limits;
  * limited implies ordered;
  * an explicit order on a shape the ordered transit kernel does not take (fewer than 2 or more
    than 128 impact parameters, fewer than 2 columns) is worked in grid order; the emission
    kernels take any shape;
  * the one-time auto ordering is tried only with >= 64 columns, never in two-stream geometry and
    never where the one-pass transit would run.

Two-stream with clouds is refused by eval_bands before planning and has no row.  The second test
holds the names that must stay reachable through pyratbay_amd.engine.  Neither needs a GPU or the
library."""
import itertools

import pytest

from pyratbay_amd.table import plan_eval_bands

GEOMETRIES = ['transit', 'emission', 'two_stream']
ROWS = [1, 2, 128, 129]                     # nlayers - itop: both sides of the ordered transit's range
NWAVES = [1, 2]
FLAGS = list(itertools.product([False, True], repeat=5))


def plan(rt_path, nrows, itop, nwave, order, limit, one_pass, continuum, cloudy):
    return plan_eval_bands(dict(rt_path=rt_path, nlayers=nrows + itop, itop=itop, nwave=nwave,
                                order_set=order, tile_limit_set=limit, one_pass=one_pass,
                                continuum=continuum), dict(cloudy=cloudy))


@pytest.mark.parametrize('itop', [0, 3])
@pytest.mark.parametrize('nwave', NWAVES)
@pytest.mark.parametrize('nrows', ROWS)
@pytest.mark.parametrize('rt_path', GEOMETRIES)
def test_truth_table(rt_path, nrows, nwave, itop):
    for order, limit, one_pass, continuum, cloudy in FLAGS:
        if rt_path == 'two_stream' and cloudy:
            continue                                    # (refused before planning)
        got = plan(rt_path, nrows, itop, nwave, order, limit, one_pass, continuum, cloudy)
        tag = (rt_path, nrows, itop, nwave, order, limit, one_pass, continuum, cloudy)
        # the form
        if cloudy:
            form = 'clouds'
        elif rt_path == 'transit' and one_pass and not continuum:
            form = 'one_pass'
        else:
            form = rt_path
        assert got.form == form, tag
        # ordered / limited
        shape_ok = rt_path != 'transit' or (nrows in (2, 128) and nwave == 2)
        ordered = order and shape_ok and rt_path != 'two_stream' and form != 'one_pass'
        assert got.ordered is ordered, tag
        assert got.limited is (ordered and limit and not cloudy), tag
        assert not got.limited or got.ordered, tag
        # what the chunk reads
        want = ('etable_ordered', 'wn_ordered', 'column_order') if ordered else \
            ('etable', 'wn', None)
        assert (got.table, got.wn, got.column) == want, tag
        assert got.may_auto_order is False, tag         # (fewer than 64 columns)


@pytest.mark.parametrize('rt_path', GEOMETRIES)
def test_auto_order_gate(rt_path):
    """The one-time ordering of the first call: at 64 columns, not at 63; not in two-stream
    geometry; not where the one-pass transit is wanted, supported and no Continuum is attached --
    whether or not the call is cloudy."""
    for nwave, one_pass, continuum, cloudy in itertools.product(
            [63, 64], [False, True], [False, True], [False, True]):
        if rt_path == 'two_stream' and cloudy:
            continue
        got = plan(rt_path, 40, 0, nwave, False, False, one_pass, continuum, cloudy)
        want = nwave == 64 and rt_path != 'two_stream' and \
            not (rt_path == 'transit' and one_pass and not continuum)
        assert got.may_auto_order is want, (rt_path, nwave, one_pass, continuum, cloudy)
        assert not got.ordered and not got.limited


# every engine.<name> that a test, a tool, bench.py or the package used before engine.py was
# split into one module per stage, and the names its description lists
FACADE = ['HiresData', 'LBL', 'LBLSpectrum', 'LineList', 'PartitionTable', 'PassBands',
          'RT_PATHS', 'SpectrumPipeline', 'StageTimer', 'TableSpectrum', 'VoigtTable', '_capi',
          '_ptr', '_stream', 'alkali_voigt_det_batch', 'blackbody_wn_2D', 'call',
          'cloudy_emission_batch', 'cloudy_transit_batch', 'deck_state_batch',
          'default_quadrature', 'dev', 'emission_flux', 'emission_flux_batch',
          'emission_observables', 'gauss_quadrature', 'hptr', 'intensity', 'internal_flux',
          'interp_ec', 'interp_ec_batch', 'loglike', 'optical_depth_transit', 'pack_raypath',
          'patchy_emission_flux', 'patchy_transit_spectrum', 'plane_parallel_optical_depth',
          'profiler_range', 'require_gpu', 'side_streams', 'table_transit_batch',
          'table_transit_supported', 'transit_path', 'transit_path_device', 'transit_spectrum',
          'transit_spectrum_batch', 'transit_spectrum_ordered', 'transmission', 'two_stream',
          'two_stream_batch']


def test_engine_is_the_front_door():
    import pyratbay_amd.engine as engine
    missing = [name for name in FACADE if getattr(engine, name, None) is None]
    assert not missing, missing
