"""Host side of the high-resolution exit of eval() (pyrat/pyrat_obj.py:331-356): the taps of the
instrument profile that ps.inst_convolution (spectrum/spec_tools.py:817-880) builds before it
convolves, and the Doppler factor of ps.rv_shift (spec_tools.py:883-907).  NumPy only; the
convolution, the shift and the sampling at the data run on the device
(csrc/pb_hires.hip, engine.HiresData)."""
import math

import numpy as np

# the reference's pc.c and pc.km
from .continuum import LS, KM

# the fused kernel stages one tile of the grid + (T - 1) / 2 samples on each side
# (csrc/pb_hires.hip kMaxTaps)
MAX_TAPS = 1025


def _gaussian_window(n, std):
    """scipy.signal.windows.gaussian(n, std) (symmetric window)."""
    x = np.arange(0, n) - (n - 1.0) / 2.0
    return np.exp(-x**2 / (2 * std * std))


def _not_a_knot(x, y, xnew):
    """The cubic spline through (x, y) with not-a-knot ends, at xnew -- what
    splev(xnew, splrep(x, y, k=3, s=0)) evaluates -- from the spline's second derivatives."""
    n = len(x)
    if n < 4:
        raise ValueError(f'a cubic spline needs 4 points, got {n}')
    h = np.diff(x)
    A = np.zeros((n, n))
    rhs = np.zeros(n)
    for i in range(1, n - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
    rhs[1:-1] = 6.0 * ((y[2:] - y[1:-1]) / h[1:] - (y[1:-1] - y[:-2]) / h[:-1])
    # third derivative continuous across x[1] and x[n-2]
    A[0, :3] = h[1], -(h[0] + h[1]), h[0]
    A[-1, -3:] = h[-1], -(h[-2] + h[-1]), h[-2]
    m = np.linalg.solve(A, rhs)
    i = np.clip(np.searchsorted(x, xnew, side='right') - 1, 0, n - 2)
    hi = h[i]
    a = (x[i + 1] - xnew) / hi
    b = (xnew - x[i]) / hi
    return a * y[i] + b * y[i + 1] + \
        ((a**3 - a) * m[i] + (b**3 - b) * m[i + 1]) * (hi * hi) / 6.0


def inst_kernel(resolution, wn=None, sampling_res=None, use_scipy=True):
    """taps[T] (T odd) of ps.inst_convolution(wn, spectrum, resolution, sampling_res): the
    convolution it returns is convolve(spectrum, taps, mode='same').  Its steps in its order: a
    Gaussian window of FWHM c / resolution sampled per km/s and normalised, the velocity width of
    a model pixel (from sampling_res, or the mean of c dwn / wn over the grid), a cubic spline
    through the window evaluated on the pixel lattice, normalised again.  With SciPy importable
    the spline is splrep/splev like the reference's (same call of the same library); without it
    (or use_scipy=False) the not-a-knot spline above, which is what splrep(k=3, s=0) is -- within
    1e-15 of the largest tap of SciPy's on the resolutions of tests/golden/g21_hires.npz."""
    pixel_dv = LS / resolution / 1e5
    n_el = int(6 * pixel_dv) + 1
    gaussian = splrep = None
    if use_scipy:
        try:
            from scipy.signal.windows import gaussian
            from scipy.interpolate import splrep, splev
        except ImportError:
            gaussian = splrep = None
    kernel = (gaussian or _gaussian_window)(n_el, std=(pixel_dv / 2.355))
    kernel /= np.sum(kernel)

    if sampling_res is None:
        if wn is None:
            raise ValueError('inst_kernel: the grid or its sampling resolution is needed')
        wn = np.asarray(wn, float)
        dv = LS / 1e5 * np.ediff1d(wn) / wn[:-1]
        rv_pix = np.abs(np.mean(dv))
    else:
        rv_pix = np.abs(LS / 1e5 / sampling_res)

    n_rv0 = int(((n_el - 1) / 2) / rv_pix)
    rv_array = np.arange(-(n_el - 1) / 2, (n_el - 1) / 2 + 1, 1)
    rv_array_mod = np.linspace(-n_rv0 * rv_pix, n_rv0 * rv_pix, int(2 * n_rv0 + 1))

    if splrep is not None:
        taps = splev(rv_array_mod, splrep(rv_array, kernel), der=0)
        taps /= sum(taps)
    else:
        # (the reference's running sum is off by up to T / 2 ulp, in a direction that depends on
        # the last bits of SciPy's taps; these taps differ there, so they take the exact sum)
        taps = _not_a_knot(rv_array, kernel, rv_array_mod)
        taps /= math.fsum(taps)
    return np.ascontiguousarray(taps, dtype=np.float64)


def doppler_factor(rv_kms):
    """wn * doppler_factor(v) is ps.rv_shift(v, wn=wn)."""
    vel = np.asarray(rv_kms, float) * KM
    return np.sqrt((1 - vel / LS) / (1 + vel / LS))


def check_data_in_grid(wn, data_wn, rv_max, span=True):
    """ValueError if a data point can leave the Doppler-shifted grid anywhere within +-rv_max
    (there the reference's interp1d raises); span=False: only the arrays and rv_max are checked."""
    wn = np.asarray(wn, float)
    data_wn = np.asarray(data_wn, float)
    if wn.ndim != 1 or len(wn) < 2 or not np.all(np.diff(wn) > 0):
        raise ValueError('HiresData: wn must be a strictly ascending grid of at least 2 samples')
    if data_wn.ndim != 1 or len(data_wn) < 1 or not np.all(np.isfinite(data_wn)):
        raise ValueError('HiresData: data_wn must be a finite 1D array with at least one point')
    if not (np.isfinite(rv_max) and 0.0 <= rv_max * KM < LS):
        raise ValueError(f'HiresData: rv_max = {rv_max} km/s')
    if not span:
        return
    lo = wn[0] * doppler_factor(-rv_max)
    hi = wn[-1] * doppler_factor(rv_max)
    if np.min(data_wn) < lo or np.max(data_wn) > hi:
        raise ValueError(
            f'HiresData: the data span {np.min(data_wn):.6f} - {np.max(data_wn):.6f} cm-1, '
            f'the grid shifted by up to +-{rv_max} km/s covers {lo:.6f} - {hi:.6f} cm-1 only')
