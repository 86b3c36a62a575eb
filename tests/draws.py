"""The seeded random acquisition generators of the randomised parity tests (tests/test_gpu_random.py) and the fuzz
(tools/auto_fuzz.py, tools/fuzz_seeds.py): plain functions of a seed, no device and no product library needed.  A draw is the
same for every seed forever -- regression seeds name draws of these generators."""
import numpy as np

from ogl_beamforming_amd import configs as cfg, params as P

S, D, I, K = P.ShaderKind, P.DataKind, P.InterpolationMode, P.AcquisitionKind


def draw(seed):
    rng = np.random.default_rng(1000 + seed)
    pick = lambda *v: v[int(rng.integers(0, len(v)))]
    interp = pick(I.Nearest, I.Linear, I.Linear, I.Cubic)
    cw = bool(rng.integers(0, 2))
    f_number = pick(0.0, 0.5, 1.0, 2.0)
    C = int(pick(8, 12, 16, 24, 40))
    samples = int(pick(256, 384, 512))
    family = pick("rca2d", "rca3d", "rca3d", "vls", "hercules", "forces", "uforces")
    common = dict(seed=seed, interp=interp, cw=cw, f_number=f_number)
    path = 0.40 * samples / 25e6 * 1540.0
    z0, z1 = 0.15 * path, 0.40 * path
    if family in ("rca2d", "rca3d", "vls"):
        A = int(pick(1, 2, 3, 5, 9))
        kind = pick(D.Int16, D.Float16, D.Float32, D.Int16Complex, D.Float32Complex)
        demod = kind in (D.Int16, D.Float16, D.Float32) and bool(rng.integers(0, 2))
        if family == "rca2d":
            points, lo, hi, orientation = (int(pick(12, 20, 33)), int(pick(12, 17)), 1), (-2e-3, 0, z0), (2e-3, 0, z1), 0x22
        else:
            points = (int(pick(6, 9, 16)), int(pick(6, 10)), int(pick(3, 5)))
            lo, hi, orientation = (-2e-3, -2e-3, z0), (2e-3, 2e-3, z1), pick(0x12, 0x21)
        depths = None
        if family == "vls":
            depths = rng.uniform(1.5 * z1, 4.0 * z1, A) * rng.choice([-1.0, 1.0], A)
        acq = cfg.rca(f"random{seed}", C, A, samples, points, lo, hi, data_kind=kind, orientation=orientation,
                      demodulate=demod, depths=depths, angles=rng.uniform(-12, 12, A) if A > 1 else None,
                      kind=K.RCA_VLS if family == "vls" else K.RCA_TPW, **common)
        bp = acq.bp
        if family == "rca3d" and A > 1 and rng.integers(0, 3) == 0:
            # per-transmit TRANSMIT orientation varies (receive fixed): still factorises
            for a in range(A):
                tx = int(pick(1, 2, 0))
                bp.transmit_receive_orientations[a] = (tx << 4) | (orientation & 0xF)
        elif family == "rca3d" and A > 1 and rng.integers(0, 4) == 0:
            # receive orientation varies too: general kernel only
            for a in range(A):
                bp.transmit_receive_orientations[a] = int(pick(0x12, 0x21))
        return acq
    A = int(pick(4, 8, 12, 16))
    kind = pick(D.Int16, D.Float16, D.Float32)
    stages = pick((S.Decode, S.DAS), (S.Demodulate, S.Decode, S.DAS))
    if family == "hercules":
        return cfg.hercules(f"random{seed}", C, A, samples, (int(pick(6, 9)), int(pick(6, 8)), int(pick(4, 6))),
                            (-1.5e-3, -1.5e-3, z0), (1.5e-3, 1.5e-3, z1), data_kind=kind, stages=stages,
                            orientation=pick(0x12, 0x21), focal=pick((0.0, np.inf), (0.0, -4.0 * z1), (4.0, np.inf)), **common)
    sparse = None
    akind = K.FORCES
    if family == "uforces":
        akind = K.UFORCES
        sparse = np.sort(rng.choice(max(C, A), A - 1, replace=False))
    return cfg.forces(f"random{seed}", C, A, samples, (int(pick(12, 20, 31)), 1, int(pick(10, 16))), (-2e-3, 0, z0), (2e-3, 0, z1),
                      data_kind=kind, stages=stages, kind=akind, sparse=sparse, **common)


def draw_separable(seed):
    """a row-column acquisition the LDS-staged kernels can take: receive and transmit on different axes, 6-20 transmits, plane or
    focused / diverging waves, ragged grids, linear / cubic interpolation, IQ or real samples (the generator of the CPU property
    test tests/test_das_select.py, with RF)"""
    rng = np.random.default_rng(2000 + seed)
    C = int(rng.choice([16, 32, 48]))
    A = int(rng.integers(6, 20))
    focused = bool(rng.integers(0, 2))
    mode = int(rng.integers(0, 4))                       # 0, 1: IQ linear; 2: IQ cubic; 3: real linear
    pitch = float(rng.choice([0.15e-3, 0.2e-3, 0.3e-3]))
    half = (C - 1) / 2 * pitch * float(rng.uniform(0.6, 2.0))
    z0 = float(rng.uniform(3e-3, 10e-3))
    z1 = z0 + float(rng.uniform(2e-3, 8e-3))
    points = (int(rng.integers(20, 110)), int(rng.integers(20, 70)), int(rng.integers(1, 3)) + 1)
    depths = rng.choice([-30e-3, -12e-3, 25e-3, 60e-3, np.inf], A) if focused else None
    return cfg.rca(f"staged{seed}", C, A, int(rng.choice([512, 1024, 2048])), points, (-half, -half * float(rng.uniform(0.5, 1.2)), z0), (half, half, z1),
                   seed=seed, orientation=int(rng.choice([0x12, 0x21])), cw=bool(rng.integers(0, 2)), f_number=float(rng.uniform(0.3, 1.5)),
                   pitch=pitch, angles=np.linspace(-float(rng.uniform(2, 20)), float(rng.uniform(2, 20)), A), depths=depths,
                   kind=K.RCA_VLS if focused else K.RCA_TPW, interp=I.Cubic if mode == 2 else I.Linear,
                   demodulate=mode != 3, data_kind=P.DataKind.Int16)


def draw_tile(seed):
    """a cubic IQ acquisition the block-staged factored kernel (das_tile.hip) can take: 2-D compounding or a view plane with tx and rx
    on one axis, a thin volume, or FORCES / UFORCES; fine to moderately coarse grids (so that blocks meet chunks that fit their window and
    chunks that do not), 4-24 plane, focused or diverging transmits, ragged tiles, short rows (terms off the end of a row: the checked
    loop), f-numbers from near field to narrow apertures, with and without coherency weighting"""
    rng = np.random.default_rng(3000 + seed)
    family = str(rng.choice(["tpw", "tpw", "vls", "volume", "forces", "uforces"]))
    C = int(rng.choice([12, 16, 24, 32]))
    pitch = float(rng.choice([0.15e-3, 0.2e-3, 0.3e-3]))
    # lateral half width: voxels of 25 um ... 250 um, and in a third of the draws around 1 mm (chunks that do not fit a window)
    coarse = rng.integers(0, 3) == 0
    half = (C - 1) / 2 * pitch * (float(rng.uniform(3.0, 6.0)) if coarse else float(rng.uniform(0.15, 1.3)))
    z0 = float(rng.uniform(2e-3, 9e-3))
    z1 = z0 + float(rng.uniform(0.4e-3, 6e-3))
    samples = int(rng.choice([384, 512, 768, 1024]))
    cw = bool(rng.integers(0, 2))
    f_number = float(rng.uniform(0.3, 1.6))
    nx, ny = int(rng.integers(40, 90 if coarse else 200)), int(rng.integers(18, 70))
    if family in ("forces", "uforces"):
        if family == "uforces":
            sparse = sorted(int(v) for v in rng.choice(np.arange(C), size=int(rng.integers(5, 9)), replace=False))
            return cfg.forces(f"tile{seed}", C, len(sparse) + 1, samples, (nx, 1, ny), (-half, 0, z0), (half, 0, z1), seed=seed, kind=K.UFORCES, sparse=sparse,
                              decode=0, interp=I.Cubic, cw=cw, f_number=f_number, pitch=pitch, stages=(S.Demodulate, S.DAS))
        return cfg.forces(f"tile{seed}", C, C, samples, (nx, 1, ny), (-half, 0, z0), (half, 0, z1), seed=seed, interp=I.Cubic, cw=cw, f_number=f_number,
                          pitch=pitch, stages=(S.Demodulate, S.Decode, S.DAS))
    A = int(rng.integers(4, 25))
    depths = rng.choice([-30e-3, -12e-3, 25e-3, 60e-3, np.inf], A) if family == "vls" else None
    if family == "volume":
        points, lo, hi = (nx, ny, int(rng.integers(2, 5))), (-half, -half * 0.3, z0), (half, half * 0.3, z1)
    else:
        points, lo, hi = (nx, ny, 1), (-half, 0, z0), (half, 0, z1)
    return cfg.rca(f"tile{seed}", C, A, samples, points, lo, hi, seed=seed, orientation=int(rng.choice([0x22, 0x22, 0x11])) if family != "volume" else 0x22,
                   cw=cw, f_number=f_number, pitch=pitch, angles=np.linspace(-float(rng.uniform(2, 18)), float(rng.uniform(2, 18)), A), depths=depths,
                   kind=K.RCA_VLS if family == "vls" else K.RCA_TPW, interp=I.Cubic, data_kind=P.DataKind.Int16)


def draw_plane(seed):
    """a VIEW PLANE through row-column / HERCULES / FORCES data, as the reference's harness beamforms one out of every dataset
    (tests/throughput.c:443-446; math.c:844-885): one voxel along z, depth on voxel y, 56-160 voxels wide so that the aligned-grid HERCULES
    kernel and the factored kernel's band walk take it; a record that ends inside the image in about half the draws (terms at the ends
    of the RF rows: the kernels' row-end instantiations), all three interpolations, with and without coherency weighting"""
    rng = np.random.default_rng(4000 + seed)
    kind = str(rng.choice(["tpw", "tpw_swapped", "vls", "hercules", "hercules", "forces"]))
    plane = "xz" if kind == "forces" else str(rng.choice(["xz", "xz", "yz"]))
    C = int(rng.choice([16, 32]))
    A = int(rng.choice([8, 16]))
    samples = int(rng.choice([512, 768, 1024]))
    k = samples / 4096.0
    nx, ny = int(rng.choice([56, 64, 96, 128, 160])), int(rng.integers(20, 72))
    reach = float(rng.uniform(0.75, 1.15))                      # > ~0.95: the deepest rows lie beyond the record
    width = float(rng.uniform(0.5, 1.1))
    lo = (-60e-3 * k * width, -60e-3 * k * width, 10e-3 * k)
    hi = (60e-3 * k * width, 60e-3 * k * width, 165e-3 * k * reach)
    fs, fd = 20e6, 5e6
    pitch = 0.25e-3 * max(k, 64.0 / C * k)
    interp = [I.Linear, I.Cubic, I.Cubic, I.Nearest][int(rng.integers(0, 4))]
    cw = bool(rng.integers(0, 2))
    f_number = float(rng.choice([0.5, 0.5, 1.0, 1.5]))
    canonical = (S.Demodulate, S.Decode, S.DAS)
    points = (nx, ny, 1)
    if kind in ("tpw", "tpw_swapped", "vls"):
        depths = np.full(A, -40e-3 * k * float(rng.uniform(0.5, 2.0))) if kind == "vls" else None
        return cfg.rca(f"plane{seed}", C, A, samples, points, lo, hi, seed=seed, interp=interp, cw=cw, f_number=f_number, pitch=pitch, fs=fs, fd=fd,
                       orientation=0x21 if kind == "tpw_swapped" else 0x12, angles=np.linspace(-float(rng.uniform(4, 18)), float(rng.uniform(4, 18)), A),
                       depths=depths, stages=canonical, plane=plane, kind=K.RCA_VLS if kind == "vls" else K.RCA_TPW)
    if kind == "hercules":
        return cfg.hercules(f"plane{seed}", C, A, samples, points, lo, hi, seed=seed, interp=interp, cw=cw, f_number=f_number, pitch=pitch, fs=fs, fd=fd,
                            stages=canonical, plane=plane)
    return cfg.forces(f"plane{seed}", C, A, samples, points, lo, hi, seed=seed, interp=interp, cw=cw, f_number=f_number, pitch=pitch, fs=fs, fd=fd,
                      stages=canonical)


def draw_paired(seed):
    """a row-column TPW volume the channel-paired form of the LDS-staged kernel can take (das_staged.hip, uniform_tables 2: 32 x 32 tiles,
    32-sample windows; the size of tests/test_gpu_staged_paired.py's cases): complex linear samples (Int16 demodulated, Int16Complex,
    Float32Complex), 16-64 channels odd and even (an odd count pairs its last channel with a zero partner), 6-140 plane transmits -- one
    group of at most 60, two groups, a few above two groups (not paired) --, counts not a multiple of 4 (padded tables), grids that are not
    multiples of 32 along either axis (ragged tiles), 1-3 planes, with and without coherency weighting, f-numbers 0.4-1.5, and in about a
    third of the draws RF rows too short for the deepest voxels (the row-end rule: those planes go to the gather kernel)"""
    rng = np.random.default_rng(5000 + seed)
    kind, demod = [(D.Int16, True), (D.Int16Complex, False), (D.Float32Complex, False)][int(rng.integers(0, 3))]
    C = int(rng.integers(16, 65))
    groups = rng.random()
    A = int(rng.integers(6, 61) if groups < 0.45 else rng.integers(61, 121) if groups < 0.92 else rng.integers(121, 141))
    orientation = int(rng.choice([0x12, 0x21]))

    def ragged(lo, hi):
        n = int(rng.integers(lo, hi))
        return n + 1 if n % 32 == 0 else n
    n_rx, n_tx = ragged(33, 130), ragged(20, 64)                  # voxels along the receive (fine) and the transmit axis
    d_rx, d_tx = float(rng.uniform(25e-6, 38e-6)), float(rng.uniform(80e-6, 140e-6))
    z = int(rng.integers(2, 4))                                   # (one plane: depth on voxel y, not a frame the separable kernels take)
    points = (n_rx, n_tx, z) if orientation == 0x12 else (n_tx, n_rx, z)
    half = (n_rx * d_rx / 2, n_tx * d_tx / 2) if orientation == 0x12 else (n_tx * d_tx / 2, n_rx * d_rx / 2)
    z0 = float(rng.uniform(6e-3, 8e-3))
    z1 = z0 + float(rng.uniform(6e-3, 11e-3))
    steer = float(rng.uniform(3.0, 9.0))
    f_number = float(rng.uniform(0.4, 1.5))

    def reach(depth):
        """RF samples (at 25 MHz) a term of a voxel at this depth can ask for: the plane wave down, the echo back across the aperture"""
        down = depth + max(half) * np.sin(np.radians(steer))
        back = np.hypot(depth, min(depth / (2.0 * f_number), (C - 1) / 2 * 0.3e-3 + max(half)))   # (the aperture, or the array's far end)
        return (down + back) / 1540.0 * 25e6 + 40.0
    short = rng.integers(0, 3) == 0                               # short rows: the deepest plane reaches beyond them, the one above it does not
    if short:
        shallower = z0 + (z1 - z0) * (z - 2) / (z - 1)
        samples = int(reach(shallower) + 0.4 * (reach(z1) - reach(shallower))) // 32 * 32
    else:
        samples = int(np.ceil(1.15 * reach(z1) / 64.0)) * 64
    acq = cfg.rca(f"paired{seed}", C, A, samples, points, (-half[0], -half[1], z0), (half[0], half[1], z1), seed=seed, orientation=orientation,
                  cw=bool(rng.integers(0, 2)), f_number=f_number, angles=np.linspace(-steer, steer, A), data_kind=kind, demodulate=demod)
    acq.notes = "short rows" if short else ""
    return acq


def draw_posed(seed, describe=False):
    """a draw of draw(), draw_plane() or draw_tile() -- chosen by the seed -- off the axes (tests/poses.py): either ROTATED, by Euler
    angles uniform in +-8 degrees applied to the grid (about its centre), to the array (about the world origin) or to both -- no exact
    zero of either matrix survives: the "any position" kernels --, or in a random SPECIAL position: each of the grid's x and y axes
    mirrored or not, 0-3 exact quarter turns about the depth axis, a z column sheared by up to +-1 mm along x and y -- the exact zeros
    survive: the fast paths on geometry that is mirrored, turned and sheared.  describe: also the unposed draw and
    (generator, "rotation" / "special", what was applied)"""
    from tests import poses
    rng = np.random.default_rng(6000 + seed)
    generator = [draw, draw_plane, draw_tile][int(rng.integers(0, 3))]
    source = int(rng.integers(0, 48))
    acq = generator(source)
    if rng.integers(0, 2) == 0:
        target = ["grid", "array", "both"][int(rng.integers(0, 3))]
        angles = rng.uniform(-8.0, 8.0, (2, 3))
        turn = [poses.rotation(1, a[1]) @ poses.rotation(0, a[0]) @ poses.rotation(2, a[2]) for a in angles]
        pieces = []
        if target in ("grid", "both"):
            pieces.append(lambda bp, V, X: (poses.about(turn[0], poses.centre(bp, V)) @ V, X))
        if target in ("array", "both"):
            pieces.append(lambda bp, V, X: (V, X @ turn[1]))
        what = (generator.__name__, "rotation", target, source, angles.round(2).tolist())
    else:
        flips = [bool(rng.integers(0, 2)) for _ in range(2)]
        quarters = int(rng.integers(0, 4))
        dx, dy = (float(v) for v in rng.uniform(-1e-3, 1e-3, 2))

        def special(bp, V, X):
            for axis in (0, 1):
                if flips[axis]:
                    V = poses.flip(V, axis)
            return poses.shear(poses.quarter_turns(bp, V, quarters), dx, dy), X
        pieces = [special]
        what = (generator.__name__, "special", flips, source, quarters, round(dx * 1e3, 3), round(dy * 1e3, 3))
    acq = poses.rewrite(acq, *pieces)
    acq.name = f"posed{seed}"
    return (acq, generator(source), what) if describe else acq


# the seeds tests/test_gpu_poses.py runs: the first 32 whose posed draw has a non-empty oracle frame with a live share at most 0.2 below
# the unposed draw's (tests/test_poses_host.py checks the list on the CPU; a seed that fails is replaced, the condition is not)
POSED_SEEDS = list(range(32))
