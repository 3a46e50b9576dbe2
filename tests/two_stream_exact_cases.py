"""What the generator of tests/golden/two_stream_exact.npz and the tests that read it must state
identically: the shapes, the classes of columns, the kernels' depth recurrence, float64 NumPy
statements of the interval formulas (the present one and the one with expm1), and the bound.

The fixture holds, per shape (L, W) and walker, the inputs ec[L, W], intervals[L - 1], temp[L] and
the 50-digit fluxes down / up [L, W] with their bolometric sums q_down / q_up [L]; per shape wn[W],
f_int[W], flux_top[W] and the trapezoid weights tw[W].  depth is NOT stored: depth_of() restates
the kernels' recurrence, and the truth was computed from the float64 dtau0 it gives.

The bound (derived from rounding counts, not from any implementation's output).  With
x_ij = h c wn_j / (k T_i):

    u_ij     = 8 + 4 x_ij / (1 - exp(-x_ij))
    scale_j  = max_i max(|down_ij|, |up_ij|, pi B_ij)                       (the 50-digit fluxes)
    bound_j  = 2^-53 (8 L scale_j + 2 pi max_i (u_ij B_ij))                 every layer of column j
    boundQ_i = sum_j |tw_j| bound_j + (6 + 3 + nparts + 1) 2^-53 sum_j |tw_j flux_ij|

u is the float64 Planck evaluation: the rounded argument of its exponential is amplified by
x e^x / (e^x - 1), plus its other roundings; a sweep of L layers carries it through twice (2 pi).
8 per layer is the project's convention, the next power of two above four times what the
corrected statement measures against the 50-digit values (1.34 per layer).  The count in boundQ:
the butterfly over a wavefront (6), the wavefronts of a workgroup (3), the parts, the product."""
import numpy as np

# the constants of csrc/pb_common.h
K_H = 6.6260755e-27
K_LS = 2.99792458e10
K_KB = 1.380658e-16
EULER = 0.5772156649015328606065120900824024

SHAPES = [(2, 8), (3, 65), (17, 257), (40, 65)]
NWALKERS = 2
RTOP_SHAPE, RTOP = (17, 257), 3          # the shape that also has the sweeps for rtop = 3
CLASSES = ('thin', 'thin_thick', 'old', 'special')
# the first interval of the columns of class 'special', cycled
FIRST = [1.0, 0.999999, 1.000001, 80.0, 40.0, 4.0, 1e-3, 1e3, 1e-16, 2.0**-30]
UNIT = 2.0**-53
PER_LAYER = 8.0
PART = 256                               # columns of a part of the net kernel


def column_class(nwave):
    """Index into CLASSES of every column: they cycle."""
    return np.arange(nwave) % len(CLASSES)


def key(L, W, walker=None):
    return f'L{L}_W{W}_' + ('' if walker is None else f'w{walker}_')


def depth_of(ec, intervals):
    """(depth[L, W], dtau0[L - 1, W]) by the kernels' recurrence in float64 without fma:
    dnext = depth + 0.5 * h[i] * (ec[i + 1] + ec[i]); dtau0 = dnext - depth (k_plane_depth with
    maxdepth = inf, k_two_stream_batch, k_two_stream_net_batch)."""
    L, W = ec.shape
    depth = np.zeros((L, W))
    dtau0 = np.empty((L - 1, W))
    for i in range(L - 1):
        depth[i + 1] = depth[i] + 0.5 * intervals[i] * (ec[i + 1] + ec[i])
        dtau0[i] = depth[i + 1] - depth[i]
    return depth, dtau0


def planck_x(wn, temp):
    """x[L, W] = h c wn / (k T)."""
    return K_H * K_LS * wn[None, :] / (K_KB * temp[:, None])


def planck(wn, temp):
    """B[L, W] in float64, the statement of _blackbody.c."""
    factor = 2 * K_H * K_LS * K_LS * wn**3
    return factor[None, :] / (np.exp(planck_x(wn, temp)) - 1.0)


def exp1(x):
    """The E1XB routine (xsf/expint.h:22-52) on an array of positive float64."""
    x = np.asarray(x, np.float64)
    out = np.empty(x.shape)
    flat, res = x.ravel(), out.ravel()
    for n, v in enumerate(flat.tolist()):
        if v <= 1.0:
            e1, r = 1.0, 1.0
            for k in range(1, 26):
                r = -r * k * v / (k + 1.0)**2
                e1 += r
                if abs(r) <= abs(e1) * 1e-15:
                    break
            res[n] = -EULER - np.log(v) + v * e1
        else:
            t0 = 0.0
            for k in range(20 + int(80.0 / v), 0, -1):
                t0 = k / (1.0 + k / (v + t0))
            res[n] = np.exp(-v) * (1.0 / (v + t0))
    return out


def exp1_units(got, want):
    """|got - want| / want in units of 2^-53; 0 where both are 0 (E1(1e3) underflows)."""
    same = got == want
    return np.where(same, 0.0, np.abs(got - want) / np.where(same, 1.0, want) / UNIT)


def two_stream(dtau0, B, f_int, flux_top, corrected=True):
    """(down, up) [L, W] of the statements of csrc/pb_two_stream.h in float64 NumPy; corrected:
    the bracket from -expm1(-dtau0), otherwise from 1 - exp(-dtau0) as the reference has it."""
    L = dtau0.shape[0] + 1
    trans = (1 - dtau0) * np.exp(-dtau0) + dtau0 * dtau0 * exp1(dtau0)
    gone = -np.expm1(-dtau0) if corrected else 1 - np.exp(-dtau0)
    down, up = np.zeros_like(B), np.zeros_like(B)
    if flux_top is not None:
        down[0] = flux_top
    for i in range(L - 1):
        bp = (B[i + 1] - B[i]) / dtau0[i]
        down[i + 1] = (trans[i] * down[i] + np.pi * B[i] * (1 - trans[i])
                       + np.pi * bp * (-2.0 / 3 * gone[i] + dtau0[i] * (1 - trans[i] / 3)))
    up[L - 1] = down[L - 1] + f_int
    for i in reversed(range(L - 1)):
        bp = (B[i + 1] - B[i]) / dtau0[i]
        up[i] = (trans[i] * up[i + 1] + np.pi * B[i + 1] * (1 - trans[i])
                 + np.pi * bp * (2.0 / 3 * gone[i] - dtau0[i] * (1 - trans[i] / 3)))
    return down, up


def bound(wn, temp, down, up):
    """bound_j [W] of the module docstring; down, up: the 50-digit fluxes of the fixture."""
    L = len(temp)
    x = planck_x(wn, temp)
    B = planck(wn, temp)
    u = 8 + 4 * x / (1 - np.exp(-x))
    scale = np.max(np.maximum(np.maximum(np.abs(down), np.abs(up)), np.pi * B), axis=0)
    return UNIT * (PER_LAYER * L * scale + 2 * np.pi * np.max(u * B, axis=0))


def bound_q(tw, bound_j, flux):
    """boundQ_i [L] of the module docstring for flux[L, W] (the 50-digit up or down)."""
    nparts = -(-len(tw) // PART)
    return (np.sum(np.abs(tw) * bound_j)
            + (6 + 3 + nparts + 1) * UNIT * np.sum(np.abs(tw[None, :] * flux), axis=1))


def walker_inputs(g, L, W, walker):
    """ec, intervals, temp of one walker of the loaded fixture g."""
    k = key(L, W, walker)
    return g[k + 'ec'], g[k + 'intervals'], g[k + 'temp']


def shared_inputs(g, L, W):
    """wn, f_int, flux_top, tw of a shape."""
    k = key(L, W)
    return g[k + 'wn'], g[k + 'f_int'], g[k + 'flux_top'], g[k + 'tw']


def truth(g, L, W, walker, rtop=0):
    """down, up [L, W], q_down, q_up [L] at 50 digits, rounded to float64."""
    k = key(L, W, walker) + ('' if rtop == 0 else f'rtop{rtop}_')
    return g[k + 'down'], g[k + 'up'], g[k + 'q_down'], g[k + 'q_up']


def cases():
    """(L, W, walker, rtop) of every set of sweeps the fixture holds."""
    out = []
    for L, W in SHAPES:
        for walker in range(NWALKERS):
            out.append((L, W, walker, 0))
            if (L, W) == RTOP_SHAPE:
                out.append((L, W, walker, RTOP))
    return out


def worst_over_bound(got, want, bound_j):
    """max |got - want| / bound over the elements, per column [W] (bound_j broadcasts over the
    layers); a non-finite element counts as infinite."""
    with np.errstate(invalid='ignore'):
        err = np.abs(got - want) / bound_j
    err = np.where(np.isfinite(got), err, np.inf)
    return np.max(err, axis=0)
