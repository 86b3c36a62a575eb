"""The ensemble filter's definitions (include/ogl_beamformer_hip.h: beamformer_hip_gram_last_frames, beamformer_hip_mix_last_frames,
beamformer_hip_clutter_projector) restated in numpy, in float64: what the host and device tests judge the library against, with the
bounds the tests use.  Frames are numpy arrays of shape (z, y, x), complex64 or float32, index 0 of a list the oldest frame; a box is
(first, count), each (x, y, z)."""
import numpy as np


def boxed(frames, box=None):
    """(K, V) array of the frames' voxels inside the box, flat box order"""
    stack = np.stack([np.asarray(f) for f in frames])
    if box is not None:
        (x0, y0, z0), (nx, ny, nz) = box
        stack = stack[:, z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]
    return stack.reshape(len(frames), -1)


def gram(frames, box=None):
    """(G, voxels, non_finite, bound): G[j, k] = sum over the voxels of the box finite in EVERY frame of conj(f_j) f_k, complex128;
    bound[j, k] = (V + 2) 2^-53 sum (|r_j| + |i_j|)(|r_k| + |i_k|) over those V voxels -- exact products, one rounding a voxel term,
    V roundings of the running sum, for the device and for this reference alike."""
    f = boxed(frames, box)
    good = np.isfinite(f.real).all(axis=0) & np.isfinite(f.imag).all(axis=0)
    g = f[:, good].astype(np.complex128)
    G = g.conj() @ g.T
    size = np.abs(g.real) + np.abs(g.imag)
    bound = (g.shape[1] + 2) * 2.0 ** -53 * (size @ size.T)
    return G, int(good.sum()), int((~good).sum()), bound


def mix(frames, W):
    """(out, bound): out[j] = sum over k of W[j, k] f_k in complex128 / float64 with plain IEEE propagation (a voxel that is not finite in
    some frame is not finite in every output), shape (M,) + the frames'; bound[j] = (2K + 2) 2^-24 sum over k of
    (|Wre| + |Wim|)(|re_k| + |im_k|) per output float (real frames: the imaginary parts are 0): the dot-product bound of a float32 chain
    of 2K terms."""
    stack = np.stack([np.asarray(f) for f in frames])
    K, shape = stack.shape[0], stack.shape[1:]
    W = np.atleast_2d(np.asarray(W))
    flat = stack.reshape(K, -1)
    if np.iscomplexobj(stack):
        f, w = flat.astype(np.complex128), W.astype(np.complex128)
        with np.errstate(invalid="ignore", over="ignore"):
            # the four real products of every term, so that 0 * NaN stays NaN in both parts as in the device's chains
            re = w.real @ f.real - w.imag @ f.imag
            im = w.imag @ f.real + w.real @ f.imag
            out = re + 1j * im
            bound = (2 * K + 2) * 2.0 ** -24 * ((np.abs(w.real) + np.abs(w.imag)) @ (np.abs(f.real) + np.abs(f.imag)))
    else:
        f, w = flat.astype(np.float64), np.real(W).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            out = w @ f
            bound = (2 * K + 2) * 2.0 ** -24 * (np.abs(w) @ np.abs(f))
    return out.reshape((W.shape[0],) + shape), bound.reshape((W.shape[0],) + shape)


def projector(G, hi, lo=0):
    """(W, eigenvalues): the eigenpairs of the Hermitian G by numpy.linalg.eigh (its upper triangle is read), eigenvalues descending;
    W = sum of u_i u_i^H over i from hi to K - lo - 1, complex128"""
    values, vectors = np.linalg.eigh(np.asarray(G, np.complex128), UPLO="U")
    values, vectors = values[::-1], vectors[:, ::-1]
    kept = vectors[:, hi:len(values) - lo]
    return kept @ kept.conj().T, values
