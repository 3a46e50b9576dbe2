"""Device-resident front-end of the hot path (host side above the C ABI).

Mirrors the call structure of the reference's Python layer for this path

    Voigt()                         pyratbay/pyrat/voigt.py:46-149
    extinction() per-layer loop     pyratbay/pyrat/extinction.py:129-213
    optical_depth()                 pyratbay/opacity/optic_depth.py:16-144
    transmission()/plane_parallel_rt()  pyratbay/spectrum/radiative_transfer.py:23-138
    spectrum()                      pyratbay/pyrat/spectrum.py:333-385

but keeps every array ([layer][wavenumber], row-major) in HBM between the stages:
ec, depth and B never travel to the host unless asked for.  torch tensors are used
only as owners of device memory; all arithmetic happens in libpbhip.so.

This module is the front door: the code lives in one module per stage (_device, lbl, columns,
batch, bands, observation, contribution, spectrum, table, retrieval, sampler, nested, modes, optimize) and every public name is re-exported here.  The modules of the
package import from those, not from here.
"""
from . import _capi                                                     # noqa: F401
from ._capi import call, hptr, f64h, i32h                               # noqa: F401
from ._device import (StageTimer, _ptr, _stream, dev, profiler_range,   # noqa: F401
                      require_gpu, side_streams)
from .lbl import LBL, LineList, PartitionTable, VoigtTable              # noqa: F401
from .columns import (RT_PATHS, _legendre_newton, blackbody_wn_2D,      # noqa: F401
                      default_quadrature, emission_flux, emission_observables, gauss_quadrature,
                      intensity, internal_flux, interp_ec, loglike, optical_depth_transit,
                      pack_raypath, patchy_emission_flux, patchy_transit_spectrum,
                      plane_parallel_optical_depth, transit_path, transit_path_device,
                      transit_spectrum, transmission, two_stream)
from . import contribution                                              # noqa: F401
from .contribution import (band_cf_host, band_contribution_cloudy_host,  # noqa: F401
                           band_contribution_host, contribution_function_host,
                           transmittance_host, transmittance_patchy_host)
from .batch import (_check_walker_tensor, _cloud_args,                  # noqa: F401
                    alkali_voigt_det_batch, band_contribution_emission_batch,
                    band_contribution_emission_cloudy_batch, band_transmittance_batch,
                    band_transmittance_cloudy_batch, cloudy_emission_batch, cloudy_transit_batch,
                    deck_state_batch, emission_flux_batch, interp_ec_batch, table_transit_batch,
                    table_transit_supported, transit_spectrum_batch, transit_spectrum_ordered,
                    two_stream_batch, two_stream_batch_star)
from .bands import HiresData, PassBands                                 # noqa: F401
from .observation import Observation, StellarGrid                       # noqa: F401
from .spectrum import LBLSpectrum, SpectrumPipeline                     # noqa: F401
from .table import TableSpectrum                                        # noqa: F401
from .retrieval import Retrieval, parse_retrieval_params                # noqa: F401
from . import sampler                                                   # noqa: F401
from .sampler import DEMC                                               # noqa: F401
from . import nested                                                    # noqa: F401
from .nested import NestedSampler                                       # noqa: F401
from . import modes                                                     # noqa: F401
from . import optimize                                                  # noqa: F401
from .optimize import LevenbergMarquardt, Optimum                       # noqa: F401
