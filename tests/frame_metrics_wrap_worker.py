"""Child process of tests/test_gpu_frame_metrics.py: frame metrics in a frame ring of BEAMFORMER_HIP_FRAME_RING_BYTES (the ring is sized
once per process), small enough that a few variants pushes wrap it.  A frame whose ring storage a newer frame has reused is no longer
scored, copied or described -- InvalidAccess, as for a tombstone --, while every frame that is still there is.
Started as python -m tests.frame_metrics_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import lib, params as P
from tests import frame_metrics_ref as ref
from tests import variants_cases as vc

E = P.LibError


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = vc.separable_volume()                                # 16 x 16 x 32 complex voxels: 64 KiB a frame
    variants = vc.candidates(acq.bp)
    frame_bytes = 16 * 16 * 32 * 8
    fit = ring // frame_bytes
    pushes = fit // 3 + 1                                      # runs of three frames; the last one does not fit behind the others
    assert fit >= 6
    frames = None
    for n in range(pushes):
        frames = lib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
        if n == 0:                                             # three frames were ever queued: a fourth cannot be scored
            four = (P.HipFrameMetrics * 4)()
            assert not L.beamformer_hip_score_last_frames(4, None, four, None) and lib.last_error()[0] == E.InvalidAccess
            assert L.beamformer_hip_score_last_frames(3, None, four, None), lib.last_error()
    info = P.HipFrameInfo()
    assert L.beamformer_hip_get_last_frame_info(C.byref(info))
    newest = int(info.frame_id)
    assert newest == 3 * pushes - 1
    # the last run went back to offset 0, over the frames of the first one
    assert int(lib.frame_info(newest - 2).device_pointer) == int(lib.frame_info(3).device_pointer) - 3 * frame_bytes
    rows, _ = lib.score_last_frames(3)
    for k in range(3):
        expected = ref.metrics(frames[k])
        assert rows[k].frame_id == newest - 2 + k and rows[k].voxels == expected["voxels"] == 16 * 16 * 32
        assert abs(rows[k].sum_abs2 - expected["sum_abs2"]) <= 2e-6 * expected["sum_abs2"]
        assert tuple(rows[k].max_index) == expected["max_index"]
    # every frame but the first run's is still its own
    alive = newest + 1 - 3
    rows, _ = lib.score_last_frames(alive)
    assert [int(r.frame_id) for r in rows] == list(range(3, newest + 1))
    assert np.array_equal(lib.copy_frame(newest - 1).view(np.uint32), frames[1].view(np.uint32))
    assert lib.copy_frame(3).shape == frames[0].shape
    # one frame further back: its storage has been reused
    out = (P.HipFrameMetrics * (alive + 1))()
    untouched = bytes(out)
    assert not L.beamformer_hip_score_last_frames(alive + 1, None, out, None) and lib.last_error()[0] == E.InvalidAccess
    assert bytes(out) == untouched
    raw = np.zeros(frame_bytes // 4, np.float32)
    for gone in (0, 1, 2):
        assert not L.beamformer_hip_copy_frame(gone, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and lib.last_error()[0] == E.InvalidAccess
        assert not L.beamformer_hip_get_frame_info(gone, C.byref(info)) and lib.last_error()[0] == E.InvalidAccess
    assert not raw.any()
    # an id that was never queued
    assert not L.beamformer_hip_get_frame_info(newest + 1, C.byref(info)) and lib.last_error()[0] == E.InvalidAccess
    print(f"reused: {pushes} runs of 3 frames of {frame_bytes} bytes in a ring of {ring}; {alive} frames still scored")


if __name__ == "__main__":
    main()
