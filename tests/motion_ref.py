"""The shift correlation's definitions (include/ogl_beamformer_hip.h: beamformer_hip_correlate_last_frames,
beamformer_hip_displacements_from_correlation) restated in numpy, in float64: what the host and device tests judge the library against,
with the bounds the tests use.  Frames are numpy arrays of shape (z, y, x), complex64 or float32, index 0 of a list the oldest frame; a
box is (first, count), each (x, y, z); a window is (Sx, Sy, Sz)."""
import numpy as np

ENTRY = np.dtype([("re", np.float64), ("im", np.float64), ("energy_reference", np.float64), ("energy_frame", np.float64), ("terms", np.uint64)])
ROW = np.dtype([("displacement", np.float32, 3), ("shift", np.int32, 3), ("coefficient", np.float32), ("phase", np.float32),
                ("fitted", np.uint32), ("at_window_edge", np.uint32)])


def correlate(frames, reference, window, boxes=None):
    """(table, bars): table of ENTRY, shape (R, K, 2 Sz + 1, 2 Sy + 1, 2 Sx + 1) -- for box b, frame k and shift s the sums over the
    voxels v of the box with v + s inside the frame, ref[v] finite and f_k[v + s] finite of conj(ref[v]) f_k[v + s], |ref[v]|^2 and
    |f_k[v + s]|^2, and their number; an entry without terms is zero.  bars: float64 of shape table.shape + (3,) -- for re and im (one
    bar), energy_reference and energy_frame: (terms + 2) 2^-53 sum (|r| + |i|)(|r| + |i|) over the terms, the two factors those of the
    product (ref and frame, ref and ref, frame and frame): exact products, one rounding a term, `terms` roundings of the running sum, for
    the device and for this reference alike."""
    stack = np.stack([np.asarray(f) for f in frames])
    K, pz, py, px = stack.shape
    Sx, Sy, Sz = (int(v) for v in window)
    boxes = [((0, 0, 0), (px, py, pz))] if boxes is None else list(boxes)
    cplx = stack.astype(np.complex128)
    finite = np.isfinite(cplx.real) & np.isfinite(cplx.imag)
    clean = np.where(finite, cplx, 0.0)
    size = np.abs(clean.real) + np.abs(clean.imag)
    table = np.zeros((len(boxes), K, 2 * Sz + 1, 2 * Sy + 1, 2 * Sx + 1), ENTRY)
    bars = np.zeros(table.shape + (3,), np.float64)
    for b, ((x0, y0, z0), (nx, ny, nz)) in enumerate(boxes):
        for sz in range(-Sz, Sz + 1):
            for sy in range(-Sy, Sy + 1):
                for sx in range(-Sx, Sx + 1):
                    # the part of the box whose shifted voxel lies inside the frame
                    xa, xb = max(x0, -sx), min(x0 + nx, px - sx)
                    ya, yb = max(y0, -sy), min(y0 + ny, py - sy)
                    za, zb = max(z0, -sz), min(z0 + nz, pz - sz)
                    if xa >= xb or ya >= yb or za >= zb:
                        continue
                    here = (slice(za, zb), slice(ya, yb), slice(xa, xb))
                    there = (slice(None), slice(za + sz, zb + sz), slice(ya + sy, yb + sy), slice(xa + sx, xb + sx))
                    good = finite[reference][here][None] & finite[there]                       # (K, ...)
                    r = np.where(good, clean[reference][here][None], 0.0)
                    f = np.where(good, clean[there], 0.0)
                    rs = np.where(good, size[reference][here][None], 0.0)
                    fs = np.where(good, size[there], 0.0)
                    axes = (1, 2, 3)
                    c = (r.conj() * f).sum(axis=axes)
                    terms = good.sum(axis=axes)
                    e = table[b, :, sz + Sz, sy + Sy, sx + Sx]
                    e["re"], e["im"] = c.real, c.imag
                    e["energy_reference"] = (r.real ** 2 + r.imag ** 2).sum(axis=axes)
                    e["energy_frame"] = (f.real ** 2 + f.imag ** 2).sum(axis=axes)
                    e["terms"] = terms
                    table[b, :, sz + Sz, sy + Sy, sx + Sx] = e
                    scale = (terms + 2) * 2.0 ** -53
                    bars[b, :, sz + Sz, sy + Sy, sx + Sx, 0] = scale * (rs * fs).sum(axis=axes)
                    bars[b, :, sz + Sz, sy + Sy, sx + Sx, 1] = scale * (rs * rs).sum(axis=axes)
                    bars[b, :, sz + Sz, sy + Sy, sx + Sx, 2] = scale * (fs * fs).sum(axis=axes)
    return table, bars


def _score(e, normalised):
    """an entry's score; negative: no candidate"""
    values = [float(e["re"]), float(e["im"]), float(e["energy_reference"]), float(e["energy_frame"])]
    if int(e["terms"]) == 0 or not np.isfinite(values).all():
        return -1.0
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.float64(values[0]) * values[0] + np.float64(values[1]) * values[1]
        if not normalised:
            return float(q)
        if not (values[2] > 0.0 and values[3] > 0.0):
            return -1.0
        return float(q / (np.float64(values[2]) * values[3]))


def displacements(tables, window, normalised=True):
    """(rows, any): the helper's rows (ROW) for an array of ENTRY whose last three axes are (2 Sz + 1, 2 Sy + 1, 2 Sx + 1), with its
    leading shape, and whether any table had a candidate"""
    S = [int(v) for v in window]
    W = [2 * v + 1 for v in S]
    tables = np.asarray(tables)
    lead = tables.shape[:-3]
    flat = tables.reshape(-1, W[0] * W[1] * W[2])
    rows = np.zeros(len(flat), ROW)
    stride = (1, W[0], W[0] * W[1])
    found = False
    for n, t in enumerate(flat):
        best, at = -1.0, 0
        for s in range(len(t)):
            q = _score(t[s], normalised)
            if q >= 0.0 and q > best:
                best, at = q, s
        if best < 0.0:
            continue
        found = True
        index = (at % W[0], at // W[0] % W[1], at // (W[0] * W[1]))
        m0 = np.sqrt(best)
        row = rows[n]
        fitted = edge = 0
        for a in range(3):
            shift, offset = index[a] - S[a], 0.0
            if S[a] > 0 and 0 < index[a] < W[a] - 1:
                below, above = _score(t[at - stride[a]], normalised), _score(t[at + stride[a]], normalised)
                if below >= 0.0 and above >= 0.0:
                    lo, hi = np.sqrt(below), np.sqrt(above)
                    den = (lo + hi) - (m0 + m0)
                    if den < 0.0:
                        offset = min(0.5, max(-0.5, 0.5 * (lo - hi) / den))
                        fitted |= 1 << a
            if S[a] > 0 and abs(shift) == S[a]:
                edge |= 1 << a
            row["shift"][a] = shift
            row["displacement"][a] = np.float32(shift + offset)
        re, im = float(t[at]["re"]), float(t[at]["im"])
        energy = float(t[at]["energy_reference"]) * float(t[at]["energy_frame"])
        row["coefficient"] = np.float32(np.sqrt(re * re + im * im) / np.sqrt(energy)) if energy > 0.0 else 0.0
        row["phase"] = np.float32(np.arctan2(im, re))
        row["fitted"], row["at_window_edge"] = fitted, edge
    return rows.reshape(lead), found
