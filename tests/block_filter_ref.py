"""The block-wise ensemble filter's definitions (include/ogl_beamformer_hip.h: beamformer_hip_gram_boxes_last_frames,
beamformer_hip_lattice_boxes, beamformer_hip_mix_field_last_frames) restated in numpy: what the host and device tests judge the library
against.  Frames are numpy arrays of shape (z, y, x), complex64 or float32, index 0 of a list the oldest frame; a box is (first, count),
each (x, y, z); a lattice is nodes, node_first, node_step, each (x, y, z); the nodes' weight tables are one array (Nz, Ny, Nx, M, K).

Two forms of the field mix.  blend() is the definition's own arithmetic on corner frames that are GIVEN -- the lerps fmaf(t, b - a, a)
in float32 with an exact fmaf --, so the device's output is judged bit for bit against corner frames the plain mix produced.
mix_field() is the whole call in float64 with a derived bound, for the loop tests that judge a chain of calls.

The exact fmaf: the product of two float32 numbers is exact in float64; adding the third is ONE rounding, to 53 bits, and TwoSum gives
what that rounding dropped.  Rounding the 53-bit sum once more to 24 bits is wrong only when the sum landed exactly on a float32 tie
while the true value lies to one side of it: there the residual decides.  (tests/warp_ref.py's fma32 documents the double rounding
this removes.)"""
import numpy as np

from tests import ensemble_ref

F32 = np.float32
FLT_MAX = np.float64(np.finfo(F32).max)
OVERFLOW_TIE = 2.0 ** 128 - 2.0 ** 103                 # halfway between FLT_MAX and 2^128: round-to-even gives infinity


def fmaf(a, b, c):
    """float32 fma on arrays, correctly rounded: exactly what fmaf(a, b, c) returns, NaN and infinities by plain IEEE"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)             # exact: 48 bits
        c = c.astype(np.float64)
        s = p + c                                                   # one rounding
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                               # TwoSum: s + e is the true value
        r = s.astype(F32)
        fine = np.isfinite(s) & np.isfinite(e) & (e != 0)
        # the sum sits exactly halfway between r and its float32 neighbour on the sum's side
        r64 = r.astype(np.float64)
        d = s - r64
        toward = np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32)
        n = np.nextafter(r, toward)
        finite_r = np.isfinite(r)
        tie = fine & finite_r & (d != 0) & ((n.astype(np.float64) - s) == d)
        r = np.where(tie & (np.sign(e) == np.sign(d)), n, r)
        # the tie at the overflow threshold: rounded to infinity, the true value below the threshold
        over = fine & ~finite_r & (np.abs(s) == OVERFLOW_TIE) & (np.sign(e) != np.sign(s))
        r = np.where(over, (np.sign(s) * FLT_MAX).astype(F32), r)
    return r.astype(F32)


# ---- boxes ----

def lattice_boxes(points, nodes, node_first, node_step, half):
    """the boxes [(first, count)] of a lattice's nodes in flat node order (jz * Ny + jy) * Nx + jx: along axis a node j sits at
    P = node_first[a] + j * node_step[a] and owns [max(0, P - half[a]), min(points[a], P + half[a] + 1)).  ValueError("InvalidAccess"):
    an entry of points or nodes that is 0, a step of 0 on an axis of several nodes, a box without a voxel;
    ValueError("BufferOverflow"): more than 1024 nodes"""
    points, nodes, node_first, node_step, half = ([int(v) for v in t] for t in (points, nodes, node_first, node_step, half))
    if 0 in points or 0 in nodes:
        raise ValueError("InvalidAccess")
    if nodes[0] * nodes[1] * nodes[2] > 1024:
        raise ValueError("BufferOverflow")
    spans = []
    for a in range(3):
        if nodes[a] > 1 and node_step[a] == 0:
            raise ValueError("InvalidAccess")
        axis = []
        for j in range(nodes[a]):
            at = node_first[a] + j * node_step[a]
            lo, hi = max(0, at - half[a]), min(points[a], at + half[a] + 1)
            if hi <= lo:
                raise ValueError("InvalidAccess")
            axis.append((lo, hi - lo))
        spans.append(axis)
    return [((sx[0], sy[0], sz[0]), (sx[1], sy[1], sz[1])) for sz in spans[2] for sy in spans[1] for sx in spans[0]]


def gram_boxes(frames, boxes):
    """[(G, voxels, non_finite, bound)] a box: tests/ensemble_ref.py's gram of each -- the definition is that the boxes do not know of
    one another"""
    return [ensemble_ref.gram(frames, box) for box in boxes]


# ---- segments ----

def segments(points, N, first, step):
    """(lower, upper, t, blended) for the voxels i = 0 .. points - 1 of one axis: the lower node, the upper node (the lower one again
    where the voxel has a single node), t as the float32 the definition names -- (float)r * (1.0f / (float)step) -- and whether the
    voxel is blended along this axis.  N == 1: node 0 everywhere, first and step are not read."""
    i = np.arange(int(points), dtype=np.int64)
    if int(N) == 1:
        zero = np.zeros(i.shape, np.int64)
        return zero, zero.copy(), np.zeros(i.shape, F32), np.zeros(i.shape, bool)
    N, first, step = int(N), int(first), int(step)
    last = first + (N - 1) * step
    blended = (i >= first) & (i < last)
    j = np.where(blended, (i - first) // step, 0)
    r = np.where(blended, (i - first) - j * step, 0)
    inv = F32(1.0) / F32(step)
    t = (r.astype(F32) * inv).astype(F32)
    lower = np.where(i < first, 0, np.where(i >= last, N - 1, j))
    return lower, np.where(blended, lower + 1, lower), np.where(blended, t, F32(0)).astype(F32), blended


def _level(values, node_axis, voxel_axis, seg, lerp):
    """one level of the blend: the node axis is consumed, every voxel along voxel_axis takes lerp(t, a, b) of its two nodes' values, or
    its single node's value as it is"""
    lower, upper, t, blended = seg
    V = values.shape[voxel_axis]
    m = np.moveaxis(values, [node_axis, voxel_axis], [0, 1])
    at = np.arange(V)
    a, b = m[lower, at], m[upper, at]                               # (V, rest...)
    shape = (V,) + (1,) * (a.ndim - 1)
    out = np.where(blended.reshape(shape), lerp(t.reshape(shape), a, b), a)
    return np.moveaxis(out, 0, voxel_axis - 1)


def _blend_parts(corners, seg3, lerp):
    x = _level(corners, 2, 6, seg3[0], lerp)                        # (Nz, Ny, M, Z, Y, X)
    y = _level(x, 1, 4, seg3[1], lerp)                              # (Nz, M, Z, Y, X)
    return _level(y, 0, 2, seg3[2], lerp)                           # (M, Z, Y, X)


def lattice_segments(shape, nodes, node_first, node_step):
    """the three axes' segments of a frame of shape (z, y, x), in the order x, y, z"""
    return [segments(shape[2 - a], nodes[a], node_first[a], node_step[a]) for a in range(3)]


def blend(corners, node_first, node_step):
    """the BLEND of the definition on given corner frames: corners (Nz, Ny, Nx, M, Z, Y, X), float32 or complex64 -- corners[jz, jy,
    jx, j] is y_c[j] of node c = (jx, jy, jz) -- -> (M, Z, Y, X) of the same type.  Each output float: lerps fmaf(t, b - a, a) in
    float32, along x, then y, then z; an axis on which the voxel has a single node contributes that node's value and no lerp."""
    corners = np.asarray(corners)
    nodes = (corners.shape[2], corners.shape[1], corners.shape[0])
    seg3 = lattice_segments(corners.shape[4:], nodes, node_first, node_step)

    def lerp(t, a, b):
        with np.errstate(invalid="ignore", over="ignore"):
            return fmaf(t, (b - a).astype(F32), a)
    if np.iscomplexobj(corners):
        corners = corners.astype(np.complex64)
        out = np.empty(corners.shape[3:], np.complex64)
        out.real = _blend_parts(np.ascontiguousarray(corners.real), seg3, lerp)
        out.imag = _blend_parts(np.ascontiguousarray(corners.imag), seg3, lerp)
        return out
    return _blend_parts(corners.astype(F32), seg3, lerp)


def mix_field(frames, W, node_first, node_step):
    """(out, bound): the whole call in float64 -- every node's mix by tests/ensemble_ref.py (its bound: the dot-product bound of a
    float32 chain of 2K terms, (2K + 2) 2^-24 S with S = sum over k of (|Wre| + |Wim|)(|re_k| + |im_k|)), blended with the definition's
    float32 t.  bound, per output float: a lerp is a convex combination, so the corners' errors pass through it at no more than their
    maximum; a level adds the rounding of b - a and of the fmaf, at most 2^-24 (|b - a| + |out|) <= 3 2^-24 max S; three levels:
    max over the nodes of (2K + 2 + 9) 2^-24 S."""
    W = np.asarray(W)
    Nz, Ny, Nx, M, K = W.shape
    stack = np.stack([np.asarray(f) for f in frames])
    cplx = np.iscomplexobj(stack)
    corners = np.empty((Nz, Ny, Nx, M) + stack.shape[1:], np.complex128 if cplx else np.float64)
    worst = np.zeros((M,) + stack.shape[1:])
    for jz in range(Nz):
        for jy in range(Ny):
            for jx in range(Nx):
                corners[jz, jy, jx], bound = ensemble_ref.mix(list(stack), W[jz, jy, jx])
                worst = np.fmax(worst, bound)
    seg3 = lattice_segments(stack.shape[1:], (Nx, Ny, Nz), node_first, node_step)

    def lerp(t, a, b):
        with np.errstate(invalid="ignore", over="ignore"):
            return a + t.astype(np.float64) * (b - a)
    if cplx:
        out = _blend_parts(np.ascontiguousarray(corners.real), seg3, lerp) + 1j * _blend_parts(np.ascontiguousarray(corners.imag), seg3, lerp)
    else:
        out = _blend_parts(corners, seg3, lerp)
    return out, worst * ((2 * K + 11) / (2 * K + 2))


# ---- the two-clutter ensemble ----

def two_clutter_ensemble(points=(32, 1, 48), K=8, seed=0, clutter=100.0, signal=1.0):
    """K complex frames of a plane (x, 1, z) whose left half (x < X / 2) and right half carry DIFFERENT rank-1 slow-time clutter --
    a_L[k] c(v) and a_R[k] c(v), a_L and a_R orthonormal, |c| about `clutter` -- over a weak signal s[k] b(v) common to both halves,
    |b| about `signal`, s of unit norm and orthogonal to a_L and a_R.  The three slow-time vectors are REAL, as the a_k of the loop of
    tests/test_gpu_ensemble.py are, and the fields complex: G[j][k] = sum conj(f_j) f_k is the transpose of the slow-time covariance
    sum f_j conj(f_k), so the projector made from G is the complex conjugate of the one that removes a complex slow-time vector, and
    only for real ones are the two the same.  Returns (frames (K, Z, 1, X) complex64, parts): parts holds the
    float64 clutter and signal fields and the three slow-time vectors.
    The lattice that goes with it, lattice(): two nodes along x, on the two voxels either side of the boundary -- a blend zone wider
    than the boundary would run one half's projector over the other half's clutter in proportion to the window --, and boxes of one
    column of Z voxels: a rank-1 clutter needs no more, and a wider box would reach across the boundary."""
    X, Y, Z = points
    assert Y == 1 and X % 2 == 0 and K >= 3
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((K, 3)))
    a_left, a_right, s = q[:, 0], q[:, 1], q[:, 2]
    c = clutter * (rng.standard_normal((Z, 1, X)) + 1j * rng.standard_normal((Z, 1, X)))
    b = signal * (rng.standard_normal((Z, 1, X)) + 1j * rng.standard_normal((Z, 1, X)))
    left = (np.arange(X) < X // 2)[None, None, :]
    slow = np.where(left[None], a_left[:, None, None, None], a_right[:, None, None, None])
    clutter_field = slow * c[None]
    signal_field = s[:, None, None, None] * b[None]
    frames = (clutter_field + signal_field).astype(np.complex64)
    return frames, {"clutter": clutter_field, "signal": signal_field, "a_left": a_left, "a_right": a_right, "s": s}


def two_clutter_lattice(points=(32, 1, 48)):
    """(nodes, node_first, node_step, half) for two_clutter_ensemble"""
    X, _, Z = points
    return (2, 1, 1), (X // 2 - 1, 0, 0), (1, 1, 1), (0, 0, Z)


def clutter_left(filtered, parts):
    """the clutter energy a filter left in `filtered` (K, Z, Y, X), measured on the slow-time directions: the energy of the filtered
    ensemble along a_L in the left half plus along a_R in the right half, sum over v of |a^H y[:, v]|^2, in float64 (the signal's own
    slow-time vector is orthogonal to both, so what is found along them is clutter the filter let through, or signal it bent there)"""
    y = np.asarray(filtered).astype(np.complex128)
    X = y.shape[3]
    left = np.tensordot(parts["a_left"].conj(), y[:, :, :, :X // 2], axes=(0, 0))
    right = np.tensordot(parts["a_right"].conj(), y[:, :, :, X // 2:], axes=(0, 0))
    return float((np.abs(left) ** 2).sum() + (np.abs(right) ** 2).sum())
