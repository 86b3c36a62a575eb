"""The cases of the READI image tests (tests/test_readi_image_host.py, tests/test_gpu_readi_image.py) and the host side of the
identity they rest on.  A plain module: no pytest marker, no device.

READI_FORCES is FORCES with transmit element tx_group * A + tx_event and every term multiplied by Hadamard[readi_group * G + tx_group]
(shaders/das.glsl:288-366); everything behind the sign is linear in the samples.  With N acquisitions, RF frame k taken under group g_k:

    sum over k of READI_frame(rf_k, g_k) = FORCES_frame(D),     D[ch][t * A + ev][s] = sum over k of H[g_k][t] * rf_k[ch][ev][s]

where the FORCES frame is that of the DERIVED acquisition: the same parameters with acquisition_kind FORCES, acquisition_count G x A and
READI off.  All cases are the `readi` case's size class: 16 channels, 512 samples, a plane of one to four 256-voxel blocks."""
import ctypes as C
import dataclasses

import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P

I = P.InterpolationMode
S = P.ShaderKind
K = P.AcquisitionKind
LO, HI = (-1e-3, 0, 5e-3), (1e-3, 0, 9e-3)          # the `readi` case's extent (tests/cases.py LO3 / HI3)

# (readi_group_count, acquisition_count, voxels); g12a1: the order-12 matrix is not symmetric, so it tells H[g][t] from H[t][g]
GEOMETRIES = {"g4a4": (4, 4, (16, 1, 16)), "g2a8": (2, 8, (24, 1, 20)), "g8a2": (8, 2, (32, 1, 32)), "g12a1": (12, 1, (24, 1, 20))}
# a permutation of 0 .. G - 1 per geometry; on g12a1 also a 9-entry list that omits groups (1, 4, 6, 8, 11) and repeats one (7)
PERMUTATIONS = {"g4a4": [2, 0, 3, 1], "g2a8": [1, 0], "g8a2": [5, 0, 7, 3, 6, 1, 4, 2], "g12a1": [7, 2, 11, 0, 5, 9, 1, 10, 3, 8, 6, 4]}
PARTIAL12 = [3, 7, 0, 10, 7, 2, 9, 5, 7]


def _forces(name, G, A, points, kind, interp, cw, seed, acquisition_kind=K.FORCES, sparse=None, readi_group=1):
    """kind "real" / "iq": Float32 / Float32Complex RF that IS the DAS input (the Decode stage is planned away: decode mode 0);
    "i16": Int16 through (Demodulate, DAS), binary16-staged"""
    common = dict(seed=seed, interp=interp, cw=cw, decode=0, readi_groups=G, readi_group=readi_group if G else 0, kind=acquisition_kind, sparse=sparse)
    if kind == "i16":
        return cfg.forces(name, 16, A, 512, points, LO, HI, stages=(S.Demodulate, S.DAS), **common)
    return cfg.forces(name, 16, A, 512, points, LO, HI, data_kind=P.DataKind.Float32Complex if kind == "iq" else P.DataKind.Float32, **common)


def image_case(geometry, interp, kind, cw=False, acquisition_kind=K.FORCES, sparse=None):
    """the READI block of a case (readi_group 1 of G)"""
    G, A, points = GEOMETRIES[geometry]
    seed = 3700 + 16 * list(GEOMETRIES).index(geometry) + 4 * int(interp) + {"real": 0, "iq": 1, "i16": 2}[kind] + 64 * cw
    name = f"readi_image_{geometry}_{interp.name.lower()}_{kind}{'_cw' if cw else ''}"
    return _forces(name, G, A, points, kind, interp, cw, seed, acquisition_kind, sparse)


def derived_case(acq, rf=None):
    """the derived acquisition of a READI block: FORCES, G x A transmits, READI off -- everything else the block's own; given, with `rf`"""
    G, A = int(acq.bp.readi_group_count), int(acq.bp.acquisition_count)
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.acquisition_kind = int(K.FORCES)
    bp.acquisition_count = G * A
    bp.readi_group_count = bp.readi_group = 0
    bp.raw_data_dimensions[0] = G * A * int(bp.sample_count)
    return dataclasses.replace(acq, name=acq.name + "_derived", bp=bp, rf=acq.rf if rf is None else rf)


def with_group(acq, group, rf=None):
    """the acquisition with a COPY of its parameters at readi_group = group (and, given, another RF frame)"""
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.readi_group = int(group)
    return dataclasses.replace(acq, bp=bp, rf=acq.rf if rf is None else rf)


def hadamard(bflib, G):
    """the library's host construction (beamformer_hip_host_hadamard), (G, G): row g entry t is the sign of tx_group t under group g"""
    h = np.zeros(G * G, np.float32)
    assert bflib.library().beamformer_hip_host_hadamard(G, h.ctypes.data_as(C.POINTER(C.c_float)))
    assert set(np.unique(h)) == {-1.0, 1.0}
    return h.reshape(G, G)


def resolved(acq, n, groups):
    G = int(acq.bp.readi_group_count)
    return [int(g) for g in groups] if groups is not None else [(int(acq.bp.readi_group) + k) % G for k in range(n)]


def decode(H, groups, inputs):
    """the across-acquisition decode of `inputs` -- (N, channels, A, samples), float32 or complex64 -- as the library fixes it: float32,
    acc = acc +- x for k = 0, 1, ... N - 1 in that order from +0.  Returns (channels, G x A, samples)."""
    inputs = np.ascontiguousarray(inputs)
    N, Cn, A, Sn = inputs.shape
    G = H.shape[0]
    x = inputs.view(np.float32).reshape(N, Cn, 1, A, -1)       # complex samples: pairs of floats
    out = np.zeros((Cn, G, A, x.shape[-1]), np.float32)
    for k in range(N):
        out = out + H[groups[k]].astype(np.float32)[None, :, None, None] * x[k]
    assert out.dtype == np.float32
    return np.ascontiguousarray(out).view(inputs.dtype).reshape(Cn, G * A, Sn)


def decoded_rf(bflib, acq, rf, groups):
    """host-decoded RF of a case whose RF is its DAS input (kinds "real" / "iq"): rows of G x A x samples per channel, the derived block's"""
    G, A, Sn = int(acq.bp.readi_group_count), int(acq.bp.acquisition_count), int(acq.bp.sample_count)
    complex_in = P.DATA_KIND_COMPLEX[int(acq.bp.data_kind)]
    frames = np.ascontiguousarray(rf)
    if complex_in:
        frames = frames.view(np.complex64)
    frames = frames.reshape(len(rf), int(acq.bp.channel_count), A, Sn)
    D = decode(hadamard(bflib, G), resolved(acq, len(rf), groups), frames)
    D = np.ascontiguousarray(D)
    return (D.view(np.float32) if complex_in else D).reshape(int(acq.bp.channel_count), -1)
