"""The warp's definition (include/ogl_beamformer_hip.h: beamformer_hip_warp_last_frames) restated in numpy: what the host and device
tests judge the library against, with the bound the tests use.  A frame is a numpy array of shape (z, y, x), complex64 or float32; its
field an array of nodes z x nodes y x nodes x x 3 float32 (displacements in voxels, components x, y, z); nodes, node_first and
node_step are (x, y, z) triples as in the C call.  The two floats of a complex voxel are sampled apart under the same weights: values
and bounds of complex frames are complex arrays whose real and imaginary parts belong to the real and imaginary floats.

warp() is the definition in float64 with the positions computed in float64 FROM THE FLOAT32 INPUTS (node_first, 1.0f / node_step and
the field are float32 numbers and enter exactly); warp_float32() follows the header operation for operation in float32.

THE BOUND, derived.  u = 2^-24.  Two parts.
ROUNDING of the weights and the sums.  A weight is computed in float32 from t: Linear, 1 - t is one rounding of a number <= 1, t none:
|w^ - w| <= c_w u with c_w = 1; Cubic, a Horner chain of three steps (an fmaf or a product each: one rounding) whose intermediates
stay below 2.5 in magnitude and are multiplied on by t <= 1: c_w = 8.  A chain of n fmaf from +0 differs from the exact sum of its own
operands by at most (n + 2) u times the sum of the terms' magnitudes (tests/spatial_ref.py has the argument).  Through the three
stages the factors compose: the device's output differs from the exact separable sum UNDER THE DEVICE'S OWN t by at most
    B_r = (1 + g_x)(1 + g_y)(1 + g_z) S(|w| + c_w u) - S(|w|),   g_a = (n_a + 2) u,
S(q) the separable sum of |f| under the weights q_x q_y q_z over the same terms (Zero: those inside the frame; Clamp: all, indices
clamped).  An axis of one point has n = 1, w = 1 exactly and fmaf(1, f, +0) = f: g = 0, c_w = 0.
POSITION.  The device's t differs from this reference's by the float32 error dp_a of p_a = v_a + d_a(v):
  * p = (float)v + d: one rounding, u (|v_a| + |d_a|);
  * the lerps of d_a: b - a and the fmaf are a rounding each of numbers <= 2 D_a and <= D_a (D_a the largest |node value| of the
    component in this frame), three levels deep, the error of a level carried through the next as a convex combination: 9 u D_a;
  * the lattice coordinate c_b = ((float)v_b - first_b) * inv_step_b: two roundings, 2 u |c_b| in units of c, taken as 3 u (|c_b| + 1),
    times the field's slope along b, at most G_ab = the largest difference of component a between neighbouring nodes along b.
    (The clamp, the floor and s = c - j are exact; d is a continuous function of c, across cells too.)
  dp_a = u [ |v_a| + |d_a| + 9 D_a + sum_b 3 (|c_b| + 1) G_ab ].
The output is a continuous, piecewise polynomial function of p under both edge modes (a weight is 0 where its tap enters or leaves
the support; Zero-mode terms leave the frame with the SAME weight they would have had, so skipping them is continuous in p only
because the index, not the weight, decides -- and the index changes where the weight is 0), so it moves by at most dp_a times a bound
on |d out / d p_a| between the two positions: |dw/dt| <= c_d (Linear 1; Catmull-Rom 1.5: the extrema of the four derivatives on
[0, 1] are 0.5, 1.39, 1.39, 0.5) for every tap of the support -- widened by one tap either side, since the device's floor may differ
from this one's by one --, the other two axes under their |w|:
    B_p = sum_a dp_a c_d E_a,   E_a = the separable sum of |f| with weight 1 on taps first_a - 1 .. first_a + n_a of axis a.
(Terms of second order in u -- dp on two axes at once, dp times the rounding -- are below 2^-40 of the sums and left out.)
ROTATION.  re' = fmaf(-wi, y, fmaf(wr, x, +0)): two roundings of numbers <= |wr||x^| + |wi||y^|, and the carried error:
    B' = 3 u (|wr| (|x| + Bx) + |wi| (|y| + By)) + |wr| Bx + |wi| By     (real frames: wi = 0 and x alone),
and likewise for im' with the parts crossed."""
import numpy as np

from tests.spatial_ref import floats_of, frame_of, share_of_bound  # noqa: F401  (share_of_bound: for the tests)

U = 2.0 ** -24
LINEAR, CUBIC = 0, 1
ZERO, CLAMP = 0, 1


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 numbers is exact in float64, the sum rounds to 53 bits and then to 24 (a
    double rounding that differs from fmaf in rare ties: inside every bound here)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def fma64(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return a * b + c


def grid_of(shape):
    """voxel indices (vx, vy, vz), each of the frame's shape (z, y, x)"""
    vz, vy, vx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    return vx, vy, vz


def lattice(shape, field, nodes, node_first, node_step, dtype, node_shift=0.0):
    """(d, c): the displacement (dx, dy, dz) at every voxel and the clamped lattice coordinates, in `dtype` (float64: the definition's
    value; float32: the header's operations).  node_shift: the mistake the host test plants, the nodes moved by that many steps."""
    N = [int(n) for n in nodes]
    field = np.asarray(field, np.float32).reshape(N[2], N[1], N[0], 3)
    v = grid_of(shape)
    f32 = dtype == np.float32
    j, s, c_all = [], [], []
    for a in range(3):
        if N[a] == 1:
            j.append(np.zeros(shape, np.int64)), s.append(None), c_all.append(np.zeros(shape, np.float64))
            continue
        first = np.float32(node_first[a])
        inv = np.float32(1.0) / np.float32(node_step[a])
        if node_shift:
            first = np.float32(first + np.float32(node_shift) * np.float32(node_step[a]))
        c = (v[a].astype(dtype) - dtype(first)) * dtype(inv)
        c = np.minimum(np.fmax(c, dtype(0)), dtype(N[a] - 1))
        cell = np.minimum(np.floor(c).astype(np.int64), N[a] - 2)
        j.append(cell), s.append(c - cell.astype(dtype)), c_all.append(c.astype(np.float64))
    lerp = (lambda t, lo, hi: fma32(t, hi - lo, lo)) if f32 else (lambda t, lo, hi: t * (hi - lo) + lo)
    d = []
    for comp in range(3):
        g = field[..., comp].astype(dtype)

        def along_x(dy, dz):
            lo = g[j[2] + dz, j[1] + dy, j[0]]
            return lo if N[0] == 1 else lerp(s[0], lo, g[j[2] + dz, j[1] + dy, j[0] + 1])

        def along_y(dz):
            lo = along_x(0, dz)
            return lo if N[1] == 1 else lerp(s[1], lo, along_x(1, dz))

        lo = along_y(0)
        d.append(lo if N[2] == 1 else lerp(s[2], lo, along_y(1)))
    return d, c_all


def weights_of(t, interpolation, dtype, bspline=False):
    """the taps' weights at fraction t, ascending tap index; float32: the header's Horner chains"""
    if interpolation == LINEAR:
        return [dtype(1) - t, t]
    if bspline:                                        # the mistake the host test plants: the cubic B-spline
        return [(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6]
    if dtype == np.float32:
        h = np.float32
        return [fma32(fma32(h(-0.5), t, h(1.0)), t, h(-0.5)) * t, fma32(fma32(h(1.5), t, h(-2.5)) * t, t, h(1.0)),
                fma32(fma32(h(-1.5), t, h(2.0)), t, h(0.5)) * t, (fma32(h(0.5), t, h(-0.5)) * t) * t]
    return [((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t]


def separable(f, taps, edge, fma, dtype):
    """the separable sum of the definition: taps[a] = (first index array, [weight arrays]) for a = x, y, z; f of shape (z, y, x, parts).
    Along x for every (y, z) row of the support, then y, then z, each a chain from +0 in ascending tap index; a term whose index lies
    outside the frame is skipped (ZERO) or its index clamped (CLAMP)."""
    Z, Y, X = f.shape[:3]
    extent = (X, Y, Z)

    def indices(a):
        first, ws = taps[a]
        out = []
        for t, w in enumerate(ws):
            i = first + t
            inside = (i >= 0) & (i < extent[a])
            out.append((np.clip(i, 0, extent[a] - 1), np.broadcast_to(np.asarray(w, dtype), first.shape)[..., None], (inside | (edge == CLAMP))[..., None]))
        return out

    ix, iy, iz = indices(0), indices(1), indices(2)
    zero = np.zeros(f.shape, dtype)
    az = zero
    for z, wz, okz in iz:
        ay = zero
        for y, wy, oky in iy:
            ax = zero
            for x, wx, okx in ix:
                ax = np.where(okx, fma(wx, f[z, y, x], ax), ax)
            ay = np.where(oky, fma(wy, ax, ay), ay)
        az = np.where(okz, fma(wz, ay, az), az)
    return az


def positions(shape, d, interpolation, dtype, bspline=False):
    """taps[a] = (first tap index, weights) of every voxel from the displacement d, and the per-axis tap count; an axis of one point:
    one tap at index 0 of weight 1"""
    v = grid_of(shape)
    extent = (shape[2], shape[1], shape[0])
    taps = []
    for a in range(3):
        if extent[a] == 1:
            taps.append((np.zeros(shape, np.int64), [np.ones(shape, dtype)]))
            continue
        p = v[a].astype(dtype) + d[a]
        i = np.floor(p)
        t = p - i
        first = i.astype(np.int64) - (1 if interpolation == CUBIC else 0)
        taps.append((first, weights_of(t, interpolation, dtype, bspline)))
    return taps


def rotate(x, rotation, fma, dtype):
    """the mix's two chains for a one-term product, on floats of shape (..., parts)"""
    wr, wi = dtype(np.complex64(rotation).real), dtype(np.complex64(rotation).imag)
    zero = dtype(0)
    if x.shape[-1] == 1:
        return fma(wr, x, zero)
    re = fma(-wi, x[..., 1], fma(wr, x[..., 0], zero))
    im = fma(wr, x[..., 1], fma(wi, x[..., 0], zero))
    return np.stack([re, im], axis=-1)


def warp(frame, field, nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1), rotation=None, interpolation=LINEAR, edge=ZERO,
         sign=1, bspline=False, node_shift=0.0):
    """(values, bound): the frame sampled at v + d(v) in complex128 (float64 for a real frame) and the bound on each float of the
    device's frame.  sign, bspline, node_shift: mistakes the host test plants (the opposite sign, cubic B-spline weights, the nodes
    off by that many steps); the bound is that of the definition whatever they say."""
    frame = np.asarray(frame)
    f = floats_of(frame)
    shape = frame.shape
    extent = (shape[2], shape[1], shape[0])
    N = [int(n) for n in nodes]
    d, c = lattice(shape, field, N, node_first, node_step, np.float64, node_shift)
    d = [sign * x for x in d]
    taps = positions(shape, d, interpolation, np.float64, bspline)
    values = separable(f, taps, edge, fma64, np.float64)

    # the rounding part: under |w| + c_w u against under |w|
    absolute = np.abs(f)
    c_w, c_d, n_taps = (8.0, 1.5, 4) if interpolation == CUBIC else (1.0, 1.0, 2)
    live = [extent[a] > 1 for a in range(3)]
    growth = np.prod([1.0 + (n_taps + 2) * U for a in range(3) if live[a]])
    plain = [(first, [np.abs(w) for w in ws]) for first, ws in taps]
    padded = [(first, [np.abs(w) + (c_w * U if live[a] else 0.0) for w in ws]) for a, (first, ws) in enumerate(taps)]
    with np.errstate(invalid="ignore"):             # (inf - inf under an infinite voxel: no bound where the value is not finite)
        bound = growth * separable(absolute, padded, edge, fma64, np.float64) - separable(absolute, plain, edge, fma64, np.float64)

    # the position part.  A voxel that is not finite and lies under the WIDENED support only adds nothing: the value is finite there,
    # and so must the device's be -- if the device's floor brought that voxel under its own support, its output would not be finite
    # and the comparison fails, as it should (frames with such voxels are warped at positions that are float32 numbers)
    absolute = np.where(np.isfinite(absolute), absolute, 0.0)
    g = np.asarray(field, np.float32).reshape(N[2], N[1], N[0], 3).astype(np.float64)
    v = grid_of(shape)
    for a in range(3):
        if not live[a]:
            continue
        D = np.abs(g[..., a]).max()
        dp = np.abs(v[a]) + np.abs(d[a]) + 9.0 * D
        for b in range(3):
            if N[b] > 1:
                dp = dp + 3.0 * (np.abs(c[b]) + 1.0) * np.abs(np.diff(g[..., a], axis=2 - b)).max()
        widened = list(plain)
        widened[a] = (taps[a][0] - 1, [np.ones(shape)] * (n_taps + 2))
        bound = bound + (U * c_d * dp)[..., None] * separable(absolute, widened, edge, fma64, np.float64)

    if rotation is not None:
        wr, wi = abs(float(np.complex64(rotation).real)), abs(float(np.complex64(rotation).imag))
        size = np.abs(values) + bound
        if f.shape[-1] == 1:
            bound = 2.0 * U * wr * size + wr * bound
        else:
            x, y, bx, by = size[..., 0], size[..., 1], bound[..., 0], bound[..., 1]
            bound = np.stack([3.0 * U * (wr * x + wi * y) + wr * bx + wi * by, 3.0 * U * (wi * x + wr * y) + wi * bx + wr * by], axis=-1)
        values = rotate(values, rotation, fma64, np.float64)
    return frame_of(values), frame_of(bound)


def warp_float32(frame, field, nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1), rotation=None, interpolation=LINEAR, edge=ZERO):
    """the header's operations one by one in float32 numpy (fma32 stands for fmaf)"""
    frame = np.asarray(frame)
    f = floats_of(frame).astype(np.float32)
    d, _ = lattice(frame.shape, field, nodes, node_first, node_step, np.float32)
    taps = positions(frame.shape, d, interpolation, np.float32)
    out = separable(f, taps, edge, fma32, np.float32)
    if rotation is not None:
        out = rotate(out, rotation, fma32, np.float32)
    return frame_of(out).astype(frame.dtype)


# ---- which path a tile takes (csrc/warp.hip, bf_kernels.h): restated, so that tests and tools can say it from the field ----

BOX_VOXELS = 4096                  # BF_WARP_BOX_VOXELS: a tile whose source box holds more takes the direct path


def tile_of(extent):
    """bf_warp_tile: the tile's voxels (x, y, z) -- eight bits dealt round-robin, x first, over the axes the tile does not yet cover"""
    log2, bits, idle, a = [0, 0, 0], 8, 0, 0
    while bits and idle < 3:
        if (1 << log2[a]) < extent[a]:
            log2[a], bits, idle = log2[a] + 1, bits - 1, 0
        else:
            idle += 1
        a = (a + 1) % 3
    return tuple(1 << v for v in log2)


def tile_boxes(shape, field, nodes=(1, 1, 1), node_first=(0, 0, 0), node_step=(1, 1, 1), interpolation=LINEAR):
    """the voxels of every tile's source box, an array (tiles z, tiles y, tiles x): per axis the lowest first tap and the highest last
    tap of the tile's voxels, each clamped into the frame, as the kernel's phase 1 reduces them (the edge mode plays no part), and
    the product of the three extents.  Positions in float64: a box may differ from the device's by a voxel an axis where a position
    lies within rounding of an integer -- callers leave a margin around BOX_VOXELS."""
    extent = (shape[2], shape[1], shape[0])
    d, _ = lattice(shape, field, nodes, node_first, node_step, np.float64)
    taps = positions(shape, d, interpolation, np.float64)
    tile = tile_of(extent)
    count = [-(-extent[a] // tile[a]) for a in range(3)]
    full = (count[2] * tile[2], count[1] * tile[1], count[0] * tile[0])
    boxes = np.ones((count[2], count[1], count[0]), np.int64)

    def per_tile(values, fill, reduce):
        padded = np.full(full, fill, np.int64)
        padded[:shape[0], :shape[1], :shape[2]] = values
        return reduce(padded.reshape(count[2], tile[2], count[1], tile[1], count[0], tile[0]), axis=(1, 3, 5))

    for a in range(3):
        first, ws = taps[a]
        lo = per_tile(np.clip(first, 0, extent[a] - 1), extent[a], np.min)
        hi = per_tile(np.clip(first + len(ws) - 1, 0, extent[a] - 1), -1, np.max)
        boxes *= hi - lo + 1
    return boxes
