"""Child process of tests/test_gpu_localisation.py: beamformer_hip_queue_localisation_map in a frame ring of
BEAMFORMER_HIP_FRAME_RING_BYTES = 1 MiB (the ring is sized once per process): 32 complex 64 x 1 x 64 frames of 32 KiB.  A burst of 16 and
a mix 16 -> 15 leave 32 KiB at the end of the ring; the peaks of the two newest frames go into a map of 128 x 1 x 100 voxels, whose
Float32 frame (51200 bytes) does not fit behind them: it wraps to offset 0, over the burst's two oldest frames.  A map of 512 x 1 x 513
voxels is a frame larger than the whole ring: FrameSizeOverflow, and nothing has changed.
Started as python -m tests.localisation_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import configs as cfg, lib, params as P
from tests import localisation_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info as newest


def binned(points, count, A):
    """the reference map of the records find_peaks returns for the `count` newest frames (complex frames: see test_gpu_localisation.py)"""
    rows, peaks, _ = lib.find_peaks_last_frames(count, 0.0, P.HIP_MAX_PEAKS_PER_FRAME)
    records = np.frombuffer(bytes(peaks), np.dtype(P.HipFramePeak))
    counts = np.zeros((points[2], points[1], points[0]), np.uint32)
    deposited, outside = ref.deposit_records(counts, records["index"], records["offset"], A)
    return counts, deposited, outside


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    assert ring == 1 << 20
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = cfg.rca("localisation_wrap", 16, 2, 256, (64, 1, 64), vc.LO, vc.HI, seed=9150, interp=P.InterpolationMode.Linear, demodulate=False,
                  data_kind=P.DataKind.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)
    rng = np.random.default_rng(9151)
    rf = rng.normal(0.0, 1.0, (16,) + acq.rf.shape).astype(acq.rf.dtype)
    W = (rng.standard_normal((15, 16)) + 1j * rng.standard_normal((15, 16))).astype(np.complex64)
    burst = lib.beamform_burst(acq.bp, rf, acq.filters).copy()                 # ids 0 .. 15 at offset 0 .. 512 KiB
    last = newest(L)
    each = int(last.size_bytes)
    base = int(last.device_pointer) - 15 * each
    assert each == 64 * 64 * 8 and int(last.frame_id) == 15 and 32 * each == ring
    first, _ = lib.mix_last_frames(16, W)                                       # ids 16 .. 30 up to 992 KiB
    assert first == 16 and int(newest(L).device_pointer) == base + 30 * each

    points = (128, 1, 100)
    grid = lib.view(points, vc.LO, (vc.HI[0], 1e-3, vc.HI[2]))
    A = lib.map_placement(list(acq.bp.das_voxel_transform), (64, 1, 64), list(grid.das_voxel_transform), points)
    lib.localisation_map_reset(points)
    rows, _ = lib.accumulate_peaks_last_frames(2, 0.0, A)
    expected, deposited, outside = binned(points, 2, A)
    counts, info = lib.localisation_map_copy()
    assert counts.tobytes() == expected.tobytes() and (int(info.deposited), int(info.outside)) == (deposited, outside) and deposited >= 16
    assert sum(int(r.deposited) for r in rows) == deposited

    # 51200 bytes do not fit the 32 KiB behind frame 30: the frame wraps to offset 0
    frame_id, _ = lib.queue_localisation_map(0.5, tag=3)
    placed = lib.frame_info(frame_id)
    assert frame_id == 31 and int(placed.device_pointer) == base and int(placed.size_bytes) == 128 * 100 * 4 and int(newest(L).frame_id) == 31
    queued = lib.copy_frame(frame_id)
    assert np.array_equal(queued.view(np.uint32), ref.queued_frame(expected, 0.5).view(np.uint32))
    assert np.array_equal(lib.copy_frame(2).view(np.uint32), burst[2].view(np.uint32))          # the burst behind the frame is still there
    for gone in (0, 1):
        raw = np.zeros(each // 4, np.float32)
        assert not L.beamformer_hip_copy_frame(gone, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and lib.last_error()[0] == P.LibError.InvalidAccess
    print(f"wrapped: a map frame of {int(placed.size_bytes)} bytes at offset 0, {deposited} deposits")

    # a map whose frame is larger than the ring
    large = (512, 1, 513)
    assert 4 * large[0] * large[2] > ring
    lib.localisation_map_reset(large)
    lib.accumulate_peaks_last_frames(1, 0.0, np.eye(3, 4))                       # the newest frame: the queued map itself, real
    before = bytes(newest(L))
    counts_before, info_before = lib.localisation_map_copy()
    out_id, ms = C.c_uint32(77), C.c_float(-1.0)
    assert not L.beamformer_hip_queue_localisation_map(1.0, 0, C.byref(out_id), C.byref(ms))
    assert lib.last_error()[0] == P.LibError.FrameSizeOverflow and out_id.value == 77 and ms.value == -1.0
    counts_after, info_after = lib.localisation_map_copy()
    assert bytes(newest(L)) == before and counts_after.tobytes() == counts_before.tobytes() and bytes(info_after) == bytes(info_before)
    assert info_after.calls == 1
    assert np.array_equal(lib.copy_frame(31).view(np.uint32), queued.view(np.uint32))
    # ... and a smaller one is queued right behind frame 31
    lib.localisation_map_reset((16, 1, 16))
    lib.accumulate_peaks_last_frames(1, 0.0, np.eye(3, 4) / 8.0)
    frame_id, _ = lib.queue_localisation_map(1.0)
    assert frame_id == 32 and int(lib.frame_info(32).device_pointer) == base + 128 * 100 * 4
    print(f"refused: a map frame of {4 * large[0] * large[2]} bytes in a ring of {ring}")


if __name__ == "__main__":
    main()
