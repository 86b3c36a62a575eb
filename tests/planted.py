"""Planted frames: blocks whose DAS sum has exactly one term a voxel, with weight exactly 1, so that the frame is the RF rearranged and
a test CHOOSES the voxels the frame operations then read -- ties, infinities, squares that overflow or underflow, subnormals, keys
that differ in one bit -- instead of taking what a push of noise happened to beamform.  The library has no call that uploads a frame
and needs none.  A plain module: no test, no device, and it never calls the library.

plane(values) and volume(values) build the acquisition; expected(values) is the frame it owes (-0 becomes +0: the accumulator starts
at +0; a NaN stays a NaN, its payload not promised); same(frame, expected) is the comparison.  The hazard frames below are functions
of a shape and a seed; each says in its docstring which sentence of which DEFINITION of include/ogl_beamformer_hip.h it aims at, and
returns the planted array with a dict of what it planned."""
import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P

SOUND, FS, K0, SAMPLES = 1540.0, 25e6, 32, 256
PITCH = 2.0 ** -12
F_NUMBER = 64.0
F32 = np.float32
FLT_MAX, FLT_MIN = np.finfo(F32).max, np.finfo(F32).tiny
SUB_MAX, SUB_MIN = np.array([0x007FFFFF, 0x00000001], np.uint32).view(F32)
PLANE, WAVE, VOLUME = (24, 1, 40), (65, 1, 3), (16, 16, 32)         # points (x, y, z) of the three shapes the hazard frames use


def _kind(values):
    values = np.asarray(values)
    if np.iscomplexobj(values):
        return np.ascontiguousarray(values, np.complex64), P.DataKind.Float32Complex
    return np.ascontiguousarray(values, F32), P.DataKind.Float32


def plane(values, name="planted_plane"):
    """values[Z, X] (or [Z, 1, X]), float32 or complex64 -> a Flash block of X channels, one transmit without a delay, received along
    the columns, on the grid (X, 1, Z): voxel (x, z) lies exactly under channel x, every other channel fails the f-number 64 aperture
    test, the nearest sample is the integer K0 + z and the apodisation is cos^2(0) = 1"""
    values, kind = _kind(values)
    if values.ndim == 3:
        assert values.shape[1] == 1
        values = values[:, 0, :]
    Z, X = values.shape
    assert 2 <= Z <= SAMPLES - K0 - 2 and X >= 2
    half = (X - 1) / 2 * PITCH
    acq = cfg.rca(name, X, 1, SAMPLES, (X, 1, Z), (-half, 0.0, K0 * SOUND / FS), (half, 0.0, (K0 + Z - 1) * SOUND / FS), seed=0,
                  data_kind=kind, interp=P.InterpolationMode.Nearest, cw=False, f_number=F_NUMBER, pitch=PITCH, fs=FS, fd=0.0,
                  orientation=0x02, angles=np.zeros(1), single=True, demodulate=False, kind=P.AcquisitionKind.Flash, noise=False, decode=0)
    rf = np.zeros((X, SAMPLES), values.dtype)
    rf[:, K0:K0 + Z] = values.T
    acq.rf = rf
    return acq


def volume(values, name="planted_volume"):
    """values[Z, Y, X] -> a HERCULES block of X receive channels and Y transmits (Y in {4, 16}: 1 / sqrt(Y) is a power of two), plane
    wave, on the grid (X, Y, Z) with the array's pitch on both axes and a z step of c / (2 fs): voxel (x, y, z) takes the one term
    (channel x, transmit y, sample K0 + z); transmit row 0 is planted times sqrt(Y), which its own weight takes back exactly"""
    values, kind = _kind(values)
    Z, Y, X = values.shape
    assert 2 <= Z <= SAMPLES - K0 - 2 and X >= 2 and Y in (4, 16)
    hx, hy = (X - 1) / 2 * PITCH, (Y - 1) / 2 * PITCH
    step = SOUND / (2 * FS)
    acq = cfg.hercules(name, X, Y, SAMPLES, (X, Y, Z), (-hx, -hy, K0 * step), (hx, hy, (K0 + Z - 1) * step), seed=0, data_kind=kind,
                       interp=P.InterpolationMode.Nearest, cw=False, f_number=F_NUMBER, pitch=PITCH, fs=FS, fd=0.0, orientation=0x12,
                       focal=(0.0, np.inf), stages=(P.ShaderKind.Decode, P.ShaderKind.DAS), decode=0)
    rf = np.zeros((X, Y, SAMPLES), values.dtype)
    rf[:, :, K0:K0 + Z] = values.transpose(2, 1, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        rf[:, 0, :] *= F32(np.sqrt(Y))
    parts = values[:, 0, :].view(F32)
    assert (np.abs(parts[np.isfinite(parts)]) <= FLT_MAX / F32(np.sqrt(Y))).all(), "a voxel of transmit row 0 overflows when planted"
    acq.rf = rf.reshape(X, Y * SAMPLES)
    return acq


def block(values, name="planted"):
    """plane() for a frame of one row of voxels along y, volume() otherwise"""
    values = np.asarray(values)
    return plane(values, name) if values.ndim == 2 or values.shape[1] == 1 else volume(values, name)


def extent(points):
    """(lo, hi): the corners of the grid plane() or volume() gives a frame of points = (x, y, z), for a map laid over it"""
    X, Y, Z = (int(v) for v in points)
    hx, hy = (X - 1) / 2 * PITCH, (Y - 1) / 2 * PITCH
    step = SOUND / FS if Y == 1 else SOUND / (2 * FS)
    return (-hx, -hy, K0 * step), (hx, hy, (K0 + Z - 1) * step)


def moved(values, shift, fill=0.0):
    """`values` (Z, Y, X) moved by shift = (x, y, z) >= 0 voxels: out[v + shift] = values[v]; what moves in is `fill`"""
    values = np.asarray(values)
    sx, sy, sz = (int(v) for v in shift)
    Z, Y, X = values.shape
    out = np.full(values.shape, fill, values.dtype)
    out[sz:, sy:, sx:] = values[:Z - sz, :Y - sy, :X - sx]
    return out


def expected(values):
    """the frame the block owes, (Z, Y, X): `values` with -0 replaced by +0"""
    values, _ = _kind(values)
    if values.ndim == 2:
        values = values[:, None, :]
    out = values.copy()
    parts = out.view(F32)
    parts[parts == 0] = 0.0
    return out


def same(frame, want):
    """bit equality wherever `want` is not NaN, NaN where it is (component by component of a complex frame)"""
    frame, want = np.ascontiguousarray(frame), np.ascontiguousarray(want)
    if frame.shape != want.shape or frame.dtype != want.dtype:
        return False
    a, b = frame.view(F32), want.view(F32)
    nan = np.isnan(b)
    return bool(np.isnan(a[nan]).all() and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)))


# ----------------------------------------------------------------------------- the hazard frames
# Every function returns (values (Z, Y, X), plan): the array to plant and a dict of what was planned -- positions are (x, y, z).

def _shape(points):
    return (int(points[2]), int(points[1]), int(points[0]))


def _flat(points, at):
    return (at[2] * points[1] + at[1]) * points[0] + at[0]


def sites(points):
    """positions of a grid by where they lie: its corners, points on its edges, on its faces and in its interior (a grid of one
    voxel along y has corners and edges only where its x-z rectangle does), in a fixed order, no position twice"""
    X, Y, Z = (int(v) for v in points)
    ends = lambda n: [0] if n == 1 else [0, n - 1]
    inner = lambda n: [0] if n == 1 else sorted({1, n // 3, n // 2, n - 2} - {0, n - 1})
    out, seen = {"corner": [], "edge": [], "face": [], "interior": []}, set()

    def take(kind, xs, ys, zs):
        for z in zs:
            for y in ys:
                for x in xs:
                    if (x, y, z) not in seen:
                        seen.add((x, y, z))
                        out[kind].append((x, y, z))
    take("corner", ends(X), ends(Y), ends(Z))
    thin = Y == 1
    take("edge", inner(X), ends(Y), ends(Z))
    take("edge", ends(X), ends(Y), inner(Z))
    if not thin:
        take("edge", ends(X), inner(Y), ends(Z))
        take("face", inner(X), inner(Y), ends(Z))
        take("face", inner(X), ends(Y), inner(Z))
        take("face", ends(X), inner(Y), inner(Z))
    take("interior", inner(X), inner(Y), inner(Z))
    return out


def _scatter(points, kinds):
    """the kinds dealt over the sites, every kind of site starting at another kind: [(position, kind index, site kind)]"""
    out = []
    for shift, (where, positions) in enumerate(sites(points).items()):
        for n, at in enumerate(positions):
            out.append((at, (n + 3 * shift) % kinds, where))
    return out


def box_numbers(plan, box=None):
    """what a frame metrics row of the box (first, count; None: the whole frame) owes by the plan alone: non_finite, gradient_pairs
    (x, y, z) and max_index -- None when the plan's largest voxels all lie outside the box"""
    points = plan["points"]
    first, count = ((0, 0, 0), points) if box is None else box
    inside = lambda at: all(f <= v < f + c for v, f, c in zip(at, first, count))
    holes = {at for at in plan["non_finite"] if inside(at)}
    pairs = []
    for axis in range(3):
        total = (count[axis] - 1) * count[(axis + 1) % 3] * count[(axis + 2) % 3]
        lost = set()
        for at in holes:
            for step in (-1, 0):
                lo = tuple(v + (step if a == axis else 0) for a, v in enumerate(at))
                hi = tuple(v + (1 if a == axis else 0) for a, v in enumerate(lo))
                if inside(lo) and inside(hi):
                    lost.add(lo)
        pairs.append(total - len(lost))
    largest = sorted((at for at in plan["largest"] if inside(at)), key=lambda at: _flat(points, at))
    return {"non_finite": len(holes), "gradient_pairs": pairs, "max_index": largest[0] if largest else None}


SPECIALS = [np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, FLT_MIN, SUB_MAX, SUB_MIN, 1.0, -1.0, 0.0, -0.0]


def specials(points, seed=0):
    """REAL.  +-inf, NaN, +-FLT_MAX, FLT_MIN, the largest and the smallest subnormal, +-1, +0 and -0 at corners, on edges, on faces and
    in the interior of seeded unit noise.  Aims at frame metrics' "A voxel that is not finite counts in non_finite and contributes to
    nothing else; a pair with such a voxel is not a pair" and "the lowest flat index (x fastest) among ties" (|+FLT_MAX| = |-FLT_MAX| are
    the largest finite magnitudes, several times over); at frame peaks' "Neighbours outside the frame and non-finite ones ... do not
    count"; at frame quantiles' "a voxel that is not [finite] counts in
    non_finite and in nothing else" and "never -0" with the subnormals as the lowest keys above 0.
    In a volume the voxels of +-FLT_MAX on transmit row y = 0 hold +-FLT_MAX / 4, what volume() can plant there.
    plan: non_finite, largest (every position of +-FLT_MAX), subnormal, zero, at (position -> value)."""
    points = tuple(int(v) for v in points)
    rng = np.random.default_rng(9100 + seed)
    values = rng.normal(0.0, 1.0, _shape(points)).astype(F32)
    values[values == 0] = F32(0.5)
    plan = {"points": points, "non_finite": [], "largest": [], "subnormal": [], "zero": [], "at": {}}
    for at, kind, _ in _scatter(points, len(SPECIALS)):
        v = F32(SPECIALS[kind])
        if points[1] > 1 and at[1] == 0 and abs(v) == FLT_MAX:
            v = v / F32(4)                    # (volume() plants transmit row 0 times sqrt(Y) <= 4)
        values[at[2], at[1], at[0]] = v
        plan["at"][at] = v
        if not np.isfinite(v):
            plan["non_finite"].append(at)
        elif abs(v) == FLT_MAX:
            plan["largest"].append(at)
        elif v == 0:
            plan["zero"].append(at)
        elif abs(v) < FLT_MIN:
            plan["subnormal"].append(at)
    return values, plan


def squares(points, seed=0):
    """COMPLEX, every component finite.  Four kinds of voxel at corners, on edges, on faces and in the interior of seeded unit noise:
    0: |re| = 2e19, so re * re is already inf; 1: re = im = 1.5e19, both squares finite and their float32 sum inf; 2: re = 1e-23, so q
    underflows to 0 on a voxel that is not zero; 3: re = 1e-20, q subnormal.  Two voxels of 1e19 + 0i tie for the largest finite
    magnitude, and a few voxels are true zeros.  Aims at "A voxel is finite when q is" of frame peaks and frame quantiles and "A voxel
    is finite when that float is" of frame metrics: kinds 0 and 1 are NON-FINITE voxels although nothing in them is, kind 2 is a zero
    for peaks and quantiles (it ties with the true zeros in the lowest plateau) and sqrtf(0) for metrics, kind 3 a subnormal key.
    plan: non_finite, largest, zero (q == 0: kind 2 and the true zeros), subnormal, kind (position -> 0..4, 4 a true zero)."""
    points = tuple(int(v) for v in points)
    rng = np.random.default_rng(9200 + seed)
    shape = _shape(points)
    values = (rng.normal(0.0, 1.0, shape) + 1j * rng.normal(0.0, 1.0, shape)).astype(np.complex64)
    plan = {"points": points, "non_finite": [], "largest": [], "zero": [], "subnormal": [], "kind": {}}
    made = [lambda s: complex(s * 2e19, 3.0), lambda s: complex(1.5e19, s * 1.5e19), lambda s: complex(s * 1e-23, 0.0),
            lambda s: complex(0.0, s * 1e-20), lambda s: complex(0.0, 0.0)]
    for n, (at, kind, _) in enumerate(_scatter(points, 5)):
        values[at[2], at[1], at[0]] = made[kind](-1.0 if n % 2 else 1.0)
        plan["kind"][at] = kind
        plan[["non_finite", "non_finite", "zero", "subnormal", "zero"][kind]].append(at)
    free = [(x, y, z) for z in range(points[2]) for y in range(points[1]) for x in range(points[0]) if (x, y, z) not in plan["kind"]]
    for at in (free[len(free) // 3], free[2 * len(free) // 3]):
        values[at[2], at[1], at[0]] = complex(1e19, 0.0)
        plan["largest"].append(at)
    return values, plan


HEIGHT = 40                                   # the plateaus' height; 40^2 = 24^2 + 32^2, so complex plateaus mix 40, 24 + 32i, 32 - 24i, -40i
_EQUALS = [complex(40, 0), complex(24, 32), complex(32, -24), complex(0, -40)]
BIG = 2 ** 24


def _colliding_squares():
    """integers (a, b, c, d) with c^2 + d^2 = a^2 + b^2 - 1 below 2^24 (so both q are exact float32) whose float32 square roots are
    the same float: two complex voxels with q_minus < q_0 and m_minus == m_0"""
    for a in range(2897, 4000):
        for b in range(1, 200):
            q = a * a + b * b
            if q >= BIG or np.sqrt(F32(q)) != np.sqrt(F32(q - 1)):
                continue
            for c in range(a, 0, -1):
                d = int(round(np.sqrt(max(0, q - 1 - c * c))))
                if c * c + d * d == q - 1:
                    return a, b, c, d
                if d > c:
                    break
    raise AssertionError("no pair of integer squares collides")


def _layout(points):
    """the plateaus of the two shapes that take them: [(name, voxels, peaks)], positions (x, y, z)"""
    line = lambda start, step, n: [tuple(s + i * d for s, d in zip(start, step)) for i in range(n)]
    if tuple(points) == PLANE:
        return [("corner", line((0, 0, 0), (1, 0, 0), 2), [(0, 0, 0)]),
                ("face", line((0, 0, 39), (1, 0, 0), 24), [(0, 0, 39)]),
                ("along z", line((5, 0, 3), (0, 0, 1), 6), [(5, 0, 3)]),
                ("along x", line((3, 0, 11), (1, 0, 0), 4), [(3, 0, 11)]),
                ("diagonal", line((10, 0, 3), (1, 0, 1), 5), [(10, 0, 3)]),
                ("antidiagonal", line((20, 0, 3), (-1, 0, 1), 4), [(20, 0, 3)]),
                ("touching", line((3, 0, 16), (1, 0, 0), 3) + line((6, 0, 17), (1, 0, 0), 3), [(3, 0, 16)]),
                ("hole", line((3, 0, 22), (1, 0, 0), 5), [(3, 0, 22), (6, 0, 22)]),
                ("block", [(x, 0, z) for z in (20, 21, 22) for x in (12, 13, 14)], [(12, 0, 20)]),
                ("alone", [(18, 0, 12)], [(18, 0, 12)]),
                ("rounding", [(11, 0, 27), (12, 0, 27)], [(11, 0, 27)]),
                ("collision", [(11, 0, 32)], [(11, 0, 32)])]
    assert tuple(points) == VOLUME, points
    return [("corner", line((0, 0, 0), (1, 0, 0), 2), [(0, 0, 0)]),
            ("face", line((0, 8, 31), (1, 0, 0), 16), [(0, 8, 31)]),
            ("along x", line((3, 3, 2), (1, 0, 0), 4), [(3, 3, 2)]),
            ("along y", line((10, 3, 2), (0, 1, 0), 5), [(10, 3, 2)]),
            ("along z", line((3, 10, 2), (0, 0, 1), 6), [(3, 10, 2)]),
            ("diagonal", line((8, 8, 5), (1, 1, 1), 5), [(8, 8, 5)]),
            ("block", [(x, y, z) for z in (12, 13, 14) for y in (2, 3, 4) for x in (2, 3, 4)], [(2, 2, 12)]),
            ("touching", line((8, 8, 12), (1, 0, 0), 3) + line((11, 9, 12), (1, 0, 0), 3), [(8, 8, 12)]),
            ("hole", line((3, 5, 17), (1, 0, 0), 5), [(3, 5, 17), (6, 5, 17)]),
            ("alone", [(11, 11, 17)], [(11, 11, 17)]),
            ("rounding", [(11, 6, 21), (12, 6, 21)], [(11, 6, 21)]),
            ("collision", [(11, 6, 26)], [(11, 6, 26)]),
            ("antidiagonal", line((5, 10, 28), (-1, 1, 0), 4), [(5, 10, 28)])]


def plateaus(points, seed=0, cplx=False):
    """INTEGER-VALUED, real or complex, on 24 x 1 x 40 or 16 x 16 x 32.  Plateaus of 2 to 27 voxels of magnitude 40 (complex: 40, 24 +
    32i, 32 - 24i and -40i mixed: one q from different components) in a background of integers of magnitude at most 8 that is full of
    ties of its own: lines along x, y, z and the diagonals, one in the frame's corner, one across a face from edge to edge, a 3 x 3 (x
    3) block, two lines of one height that touch only diagonally (one plateau: one peak), a line with a NaN voxel inside (two: "non-
    finite ones ... do not count").  Aims at frame peaks' "q > q_n when n's flat index is below i, q >= q_n when it is above", "of a
    plateau, the voxel of the lowest flat index is one" and "No two adjacent voxels are both peaks".  The offsets: the first voxel of
    a line has m_0 = m_plus > m_minus along the line, offset exactly +0.5; "alone" is one voxel whose six axis neighbours are all 2:
    fitted, numerator 0, offset -0 (0.5f * 0 over a negative den).  A peak's neighbour at -1 has a LOWER q, so the mirror m_minus =
    m_0 > m_plus and den == 0 cannot be planted with exact magnitudes; they can with rounded ones.  "rounding": 2^24 - 1, 2^24, 2^24
    along x -- (m_minus + m_plus) rounds to 2^25 = m_0 + m_0: den == 0, "Axes that are not fitted carry 0" -- and its two voxels of
    2^24 tie for max_abs ("the lowest flat index ... among ties").  "collision" (complex only): two neighbours along x whose q differ
    by one unit and whose sqrtf are the same float, m_minus == m_0 with q_minus < q_0: offset exactly -0.5.
    plan: peaks (sorted by flat index: the peaks at threshold 40), plateaus (name -> voxels), non_finite, largest, offsets
    (position -> (axis, offset, fitted)): the planned fits."""
    points = tuple(int(v) for v in points)
    rng = np.random.default_rng(9300 + seed + (50 if cplx else 0))
    shape = _shape(points)
    if cplx:
        values = (rng.integers(-5, 6, shape) + 1j * rng.integers(-5, 6, shape)).astype(np.complex64)
    else:
        values = rng.integers(-8, 9, shape).astype(F32)
    plan = {"points": points, "peaks": [], "plateaus": {}, "non_finite": [], "largest": [], "offsets": {}}

    def put(at, v):
        values[at[2], at[1], at[0]] = v
    a, b, c, d = _colliding_squares()
    n = 0
    for name, voxels, peaks in _layout(points):
        if name == "collision" and not cplx:
            continue
        plan["plateaus"][name] = voxels
        plan["peaks"] += peaks
        for at in voxels:
            n += 1
            put(at, _EQUALS[n % 4] if cplx else F32(HEIGHT if n % 2 else -HEIGHT))
        first = voxels[0]
        left, right = (first[0] - 1, first[1], first[2]), (first[0] + 1, first[1], first[2])
        if name == "hole":
            hole = voxels[2]
            put(hole, complex(np.nan, np.nan) if cplx else np.nan)
            plan["non_finite"].append(hole)
        elif name == "alone":
            for axis in range(3):
                for step in (-1, 1):
                    at = tuple(v + (step if k == axis else 0) for k, v in enumerate(first))
                    if 0 <= at[axis] < points[axis]:
                        put(at, complex(0, -2) if cplx else F32(-2 * step))
                if points[axis] > 1:
                    plan["offsets"][(first, axis)] = (-0.0, True)
        elif name == "rounding":
            put(left, complex(0, BIG - 1) if cplx else F32(BIG - 1))
            put(first, complex(-BIG, 0) if cplx else F32(-BIG))
            put(voxels[1], complex(0, BIG) if cplx else F32(BIG))
            plan["largest"] = list(voxels)
            plan["offsets"][(first, 0)] = (0.0, False)
        elif name == "collision":
            put(left, complex(c, -d))
            put(first, complex(-b, a))
            put(right, complex(1, 1))
            plan["offsets"][(first, 0)] = (-0.5, True)
        elif name in ("along x", "along y", "along z"):
            plan["offsets"][(first, "xyz".index(name[-1]))] = (0.5, True)
    plan["peaks"].sort(key=lambda at: _flat(points, at))
    return values, plan


def bits_to_float(bits):
    return np.asarray(bits, np.uint32).view(F32)


RADIX_TIE = 0x3F800000
RADIX_GROUPS = {"bit 0": (0x40000000, 0x40000001), "bit 10": (0x41000000, 0x41000400), "bit 20": (0x42000000, 0x42100000)}
RADIX_LOWEST, RADIX_HIGHEST = 0x00000123, 0x7F712345      # coarse bins 0 (a subnormal) and 2039 (the last finite one)


def radix(seed=0):
    """REAL, 16 x 16 x 32 = 8192 voxels, the values chosen by their bits, the signs at random (q is fabsf).  Half the frame is one
    value (1.0); three groups of two keys that differ in bit 0 only, in bit 10 only and in bit 20 only, 3 to 9 voxels a key; one
    voxel in coarse bin 0 (a subnormal) and one in bin 2039; the rest has its own random key each between 2^-8 and 2^-1, every
    position shuffled.  Aims at frame quantiles' "a radix select on bits 30..20, 19..10 and 9..0 of q", "below = #{q < value} and
    equal = #{q == value}, so below <= r < below + equal" and the rank formula: the fractions of the plan put a rank on the first
    and on the last index of the tie and on both sides of every key of every group, so that each pass has to pick the right digit
    and the next one start from the right remainder.
    plan: ranks (in ascending order), fractions (lists of at most 16, covering the ranks), groups (name -> the ranks of its two
    keys' first voxels), tie (first rank, last rank)."""
    points = VOLUME
    rng = np.random.default_rng(9400 + seed)
    n = int(np.prod(points))
    keys = [RADIX_TIE] * (n // 2) + [RADIX_LOWEST, RADIX_HIGHEST]
    for m, (low, high) in zip(((3, 5), (4, 9), (7, 3)), RADIX_GROUPS.values()):
        keys += [low] * m[0] + [high] * m[1]
    rest = rng.choice(np.arange(0x3B800000, 0x3F000000, dtype=np.int64), n - len(keys), replace=False)
    keys = np.concatenate([np.asarray(keys, np.int64), rest])
    assert len(keys) == n
    ordered = np.sort(keys)
    signs = rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    values = bits_to_float(keys.astype(np.uint32) | signs)[rng.permutation(n)].reshape(_shape(points)).copy()
    first = lambda k: int(np.searchsorted(ordered, k, side="left"))
    last = lambda k: int(np.searchsorted(ordered, k, side="right")) - 1
    ranks = {0, n - 1, first(RADIX_TIE) - 1, first(RADIX_TIE), last(RADIX_TIE), last(RADIX_TIE) + 1}
    groups = {}
    for name, (low, high) in RADIX_GROUPS.items():
        ranks |= {first(low) - 1, first(low), last(low), first(high), last(high), last(high) + 1}
        groups[name] = (first(low), first(high))
    ranks = sorted(r for r in ranks if 0 <= r < n)
    fractions = [r / (n - 1) for r in ranks]
    plan = {"points": points, "ranks": ranks, "fractions": [fractions[i:i + 16] for i in range(0, len(fractions), 16)], "groups": groups,
            "tie": (first(RADIX_TIE), last(RADIX_TIE)), "non_finite": [], "keys": ordered.astype(np.uint32)}
    return values, plan


def integers(K, points, seed=0, cplx=False):
    """K frames, real or complex, whose components are integers of magnitude at most 64: every product and every sum of gram, mix,
    autocorrelate, convolve (integer taps, ZERO mode) and correlate over at most 17 frames and 8192 voxels is then below 2^53 and
    -- where the result is a float32 -- below 2^24, so exact in float32 and in double IN ANY ORDER: the result is the int64 one, bit
    for bit, whatever the kernel's order of summation or use of fused multiply-adds.  (K, Z, Y, X); every frame its own draw."""
    rng = np.random.default_rng(9500 + seed + (50 if cplx else 0))
    shape = (int(K),) + _shape(points)
    if cplx:
        return (rng.integers(-64, 65, shape) + 1j * rng.integers(-64, 65, shape)).astype(np.complex64)
    return rng.integers(-64, 65, shape).astype(F32)
