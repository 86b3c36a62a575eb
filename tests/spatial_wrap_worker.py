"""Child process of tests/test_gpu_spatial.py: beamformer_hip_convolve_last_frames in a frame ring of BEAMFORMER_HIP_FRAME_RING_BYTES =
1 MiB (the ring is sized once per process): 32 complex 64 x 1 x 64 frames of 32 KiB.  A burst of 16 and a mix 16 -> 15 leave 32 KiB at
the end of the ring, and the filtered copies of the 2 newest frames wrap to offset 0, clear of their sources; another burst of 16 and a
mix 16 -> 14 then fill the ring to its last byte, and the 32 newest frames filtered -- a run of the whole ring -- would lie on every one
of its own sources: FrameSizeOverflow, and nothing has changed; the 14 newest then wrap to offset 0 under three passes in Normalised
mode, whose scratch is the library's own.
Started as python -m tests.spatial_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import configs as cfg, lib, params as P
from tests import spatial_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info as newest


def share_of_bound(out, frames, taps, mode):
    worst = 0.0
    for got, frame in zip(out, frames):
        values, bound = ref.convolve(frame, taps, mode)
        w, inside = ref.share_of_bound(got, values, bound)
        assert inside, w
        worst = max(worst, w)
    return worst


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    assert ring == 1 << 20
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = cfg.rca("spatial_wrap", 16, 2, 256, (64, 1, 64), vc.LO, vc.HI, seed=8950, interp=P.InterpolationMode.Linear, demodulate=False,
                  data_kind=P.DataKind.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)
    rng = np.random.default_rng(8951)
    rf = rng.normal(0.0, 1.0, (16,) + acq.rf.shape).astype(acq.rf.dtype)
    W = (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))).astype(np.complex64)
    taps = [rng.uniform(0.1, 1.0, 9).astype(np.float32), rng.uniform(0.1, 1.0, 3).astype(np.float32), rng.uniform(0.1, 1.0, 5).astype(np.float32)]
    burst = lib.beamform_burst(acq.bp, rf, acq.filters).copy()                 # ids 0 .. 15 at offset 0 .. 512 KiB
    last = newest(L)
    each = int(last.size_bytes)
    base = int(last.device_pointer) - 15 * each
    assert each == 64 * 64 * 8 and int(last.frame_id) == 15 and 32 * each == ring

    # 16 -> 15: ids 16 .. 30 up to 992 KiB; the filtered copies of the 2 newest (64 KiB) do not fit behind them: the run wraps to offset 0
    first, _ = lib.mix_last_frames(16, W[:15])
    mixed = lib.get_last_frames(acq.bp, 15).copy()
    assert first == 16 and int(newest(L).device_pointer) == base + 30 * each
    first, _ = lib.convolve_last_frames(2, taps[:1] + [None, taps[2]])
    out = lib.get_last_frames(acq.bp, 2).copy()
    assert first == 31 and int(lib.frame_info(31).device_pointer) == base and int(newest(L).device_pointer) == base + each
    wrapped = share_of_bound(out, mixed[13:], taps[:1] + [None, taps[2]], 0)
    print(f"wrapped: two filtered frames at offset 0, worst error {wrapped:.4f} of its bound")
    assert np.array_equal(lib.copy_frame(29).view(np.uint32), mixed[13].view(np.uint32))        # a source of the run
    assert np.array_equal(lib.copy_frame(2).view(np.uint32), burst[2].view(np.uint32))          # the burst behind the run is still there
    for gone in (0, 1):
        raw = np.zeros(each // 4, np.float32)
        assert not L.beamformer_hip_copy_frame(gone, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and lib.last_error()[0] == P.LibError.InvalidAccess
        assert not L.beamformer_hip_get_frame_info(gone, C.byref(P.HipFrameInfo()))

    # a burst (ids 33 .. 48, 64 .. 576 KiB) and a mix 16 -> 14 (ids 49 .. 62) fill the ring to its last byte
    lib.beamform_burst(acq.bp, rf, acq.filters)
    first, _ = lib.mix_last_frames(16, W[:14])
    assert first == 49 and int(newest(L).device_pointer) == base + 31 * each and int(newest(L).frame_id) == 62
    # the 32 newest frames, ids 31 .. 62, are the whole ring: their filtered copies would lie on every one of them
    newest_frames = lib.get_last_frames(acq.bp, 32).copy()
    out_id, ms = C.c_uint32(77), C.c_float(-1.0)
    before = bytes(newest(L))
    pointers = (C.POINTER(C.c_float) * 3)(*[h.ctypes.data_as(C.POINTER(C.c_float)) for h in taps])
    counts = (C.c_uint32 * 3)(9, 3, 5)
    for mode in (0, 1):
        assert not L.beamformer_hip_convolve_last_frames(32, pointers, counts, mode, 0, C.byref(out_id), C.byref(ms))
        assert lib.last_error()[0] == P.LibError.FrameSizeOverflow and out_id.value == 77 and ms.value == -1.0
    # as if it had not been called: the counter, the 32 newest frames, the ids and the place of what follows
    assert bytes(newest(L)) == before and int(newest(L).frame_id) == 62
    assert lib.get_last_frames(acq.bp, 32).tobytes() == newest_frames.tobytes()
    assert np.array_equal(lib.copy_frame(31).view(np.uint32), out[0].view(np.uint32))
    # the 14 newest frames wrap to offset 0, clear of their sources: three passes, Normalised (the scratch run and two D fields)
    first, _ = lib.convolve_last_frames(14, taps, P.HipSpatialMode.Normalised)
    assert first == 63 and int(lib.frame_info(63).device_pointer) == base and int(newest(L).device_pointer) == base + 13 * each
    again = share_of_bound(lib.get_last_frames(acq.bp, 14).copy(), newest_frames[18:], taps, 1)
    assert lib.get_last_frames(acq.bp, 28)[:14].tobytes() == newest_frames[18:].tobytes()        # the sources, untouched by the passes
    print(f"refused: a run of {32 * each} bytes over its own 32 sources in a ring of {ring}; wrapped twice, {again:.4f} of the bound")


if __name__ == "__main__":
    main()
