"""Child process of tests/test_gpu_burst.py: bursts in a frame ring of BEAMFORMER_HIP_FRAME_RING_BYTES (the ring is sized once per
process).  A burst that would straddle the end of the ring starts again at offset 0, contiguous, and stays exportable.
Started as python -m tests.burst_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import lib, params as P
from tests import cases
from tests.frame_info import newest_info as newest


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = cases.make("config1_small")
    one = lib.beamform(acq.bp, acq.rf, acq.filters)            # the ring's first frame: offset 0
    first = newest(L)
    frame_bytes, base = int(first.size_bytes), int(first.device_pointer)
    n = ring // frame_bytes * 5 // 8                            # two such bursts do not fit the ring
    assert 2 <= n <= P.HIP_MAX_BURST_FRAMES and (2 * n + 1) * frame_bytes > ring >= (n + 1) * frame_bytes
    rng = np.random.default_rng(5)
    rf = np.clip(np.rint(rng.normal(0, 1000.0, (n,) + acq.rf.shape)), -32000, 32000).astype(acq.rf.dtype)
    a = lib.beamform_burst(acq.bp, rf, acq.filters).copy()
    assert int(newest(L).device_pointer) == base + n * frame_bytes          # behind the single frame, contiguous
    b = lib.beamform_burst(acq.bp, rf, acq.filters).copy()
    assert int(newest(L).device_pointer) == base + (n - 1) * frame_bytes    # the whole burst went back to offset 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a[0], a[1]) and a.shape[1:] == one.shape
    # the records the second burst overwrote are gone; the newest n are all there
    both = np.zeros(2 * n * frame_bytes // 4, np.float32)
    assert L.beamformer_get_last_frames(both.ctypes.data_as(C.c_void_p), both.nbytes, 2 * n)
    # a burst the ring cannot hold is refused and takes no frame id
    before = newest(L).frame_id
    too_many = ring // frame_bytes + 1
    if too_many <= P.HIP_MAX_BURST_FRAMES:
        big = np.zeros((too_many,) + acq.rf.shape, acq.rf.dtype)
        assert not L.beamformer_hip_push_data_burst_with_compute(big.ctypes.data_as(C.c_void_p), big[0].nbytes, too_many, 0, 0)
        assert lib.last_error()[0] == P.LibError.FrameSizeOverflow
        lib.beamform(acq.bp, acq.rf, acq.filters)
        assert newest(L).frame_id == before + 1
    print(f"wrapped: {n} frames of {frame_bytes} bytes twice in a ring of {ring}")


if __name__ == "__main__":
    main()
