"""Child process of tests/test_gpu_tracks.py: beamformer_hip_queue_track_map in a frame ring of BEAMFORMER_HIP_FRAME_RING_BYTES = 1 MiB
(the ring is sized once per process): 32 complex 64 x 1 x 64 frames of 32 KiB.  A burst of 16 and a mix 16 -> 15 leave 32 KiB at the end
of the ring; the peaks of the two newest frames are paired into a track map of 128 x 1 x 100 voxels, whose Float32 frame (51200 bytes)
does not fit behind them: it wraps to offset 0, over the burst's two oldest frames.  A track map of 512 x 1 x 513 voxels is a frame
larger than the whole ring: FrameSizeOverflow, and nothing has changed.
Started as python -m tests.tracks_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import configs as cfg, lib, params as P
from tests import tracks_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info as newest


def paired(points, count, A, reach):
    """the reference map of the records find_peaks returns for the `count` newest frames (complex frames: see test_gpu_tracks.py)"""
    rows, peaks, _ = lib.find_peaks_last_frames(count, 0.0, P.HIP_MAX_PEAKS_PER_FRAME)
    records = np.frombuffer(bytes(peaks), np.dtype(P.HipFramePeak))
    lists = [(records[int(r.first):int(r.first) + int(r.stored)]["index"], records[int(r.first):int(r.first) + int(r.stored)]["offset"]) for r in rows]
    counts, sums = ref.empty_map(points)
    want, numbers = ref.pair_records(lists, A, reach, counts=counts, sums=sums)
    return counts, sums, want, numbers


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    assert ring == 1 << 20
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = cfg.rca("tracks_wrap", 16, 2, 256, (64, 1, 64), vc.LO, vc.HI, seed=9350, interp=P.InterpolationMode.Linear, demodulate=False,
                  data_kind=P.DataKind.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)
    rng = np.random.default_rng(9351)
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
    lib.track_map_reset(points)
    rows, pairs, _ = lib.pair_peaks_last_frames(2, 0.0, A, 6.0, P.HIP_MAX_PEAKS_PER_FRAME, deposit=True)
    counts, sums, want, numbers = paired(points, 2, A, 6.0)
    got_counts, got_sums, info = lib.track_map_copy()
    assert bytes(pairs) == want.tobytes() and got_counts.tobytes() == counts.tobytes() and got_sums.tobytes() == sums.tobytes()
    deposited = numbers[0]["deposited"]
    assert (int(info.pairs), int(info.deposited), int(rows[0].deposited)) == (len(want), deposited, deposited) and deposited >= 16

    # 51200 bytes do not fit the 32 KiB behind frame 30: the frame wraps to offset 0
    frame_id, _ = lib.queue_track_map(3, 0.5, tag=3)
    placed = lib.frame_info(frame_id)
    assert frame_id == 31 and int(placed.device_pointer) == base and int(placed.size_bytes) == 128 * 100 * 4 and int(newest(L).frame_id) == 31
    queued = lib.copy_frame(frame_id)
    assert np.array_equal(queued.view(np.uint32), ref.queued_frame(counts, sums, 3, 0.5).view(np.uint32))
    assert np.array_equal(lib.copy_frame(2).view(np.uint32), burst[2].view(np.uint32))          # the burst behind the frame is still there
    for gone in (0, 1):
        raw = np.zeros(each // 4, np.float32)
        assert not L.beamformer_hip_copy_frame(gone, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and lib.last_error()[0] == P.LibError.InvalidAccess
    print(f"wrapped: a track map frame of {int(placed.size_bytes)} bytes at offset 0, {deposited} pairs deposited")

    # a map whose frame is larger than the ring
    large = (512, 1, 513)
    assert 4 * large[0] * large[2] > ring
    lib.track_map_reset(large)
    lib.pair_peaks_last_frames(2, 0.0, np.eye(3, 4), 2.0, 4096, deposit=True)   # the two newest frames: a mix, and the queued map itself
    before = bytes(newest(L))
    map_before = lib.track_map_copy()
    out_id, ms = C.c_uint32(77), C.c_float(-1.0)
    assert not L.beamformer_hip_queue_track_map(0, 1.0, 1, 0, C.byref(out_id), C.byref(ms))
    assert lib.last_error()[0] == P.LibError.FrameSizeOverflow and out_id.value == 77 and ms.value == -1.0
    map_after = lib.track_map_copy()
    assert bytes(newest(L)) == before and all(bytes(a) == bytes(b) if not isinstance(a, np.ndarray) else a.tobytes() == b.tobytes()
                                              for a, b in zip(map_after, map_before))
    assert map_after[2].calls == 1
    assert np.array_equal(lib.copy_frame(31).view(np.uint32), queued.view(np.uint32))
    # ... and a smaller one is queued right behind frame 31
    lib.track_map_reset((16, 1, 16))
    lib.pair_peaks_last_frames(2, 0.0, np.eye(3, 4) / 8.0, 2.0, 4096, deposit=True)
    frame_id, _ = lib.queue_track_map(4, 1.0)
    assert frame_id == 32 and int(lib.frame_info(32).device_pointer) == base + 128 * 100 * 4
    print(f"refused: a track map frame of {4 * large[0] * large[2]} bytes in a ring of {ring}")


if __name__ == "__main__":
    main()
