"""Child process of tests/test_gpu_variants.py: variants pushes in a frame ring of BEAMFORMER_HIP_FRAME_RING_BYTES (the ring is sized
once per process).  A run of frames that would straddle the end of the ring starts again at offset 0, contiguous, and stays exportable;
a run the ring cannot hold is refused and takes no frame id.
Started as python -m tests.variants_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import lib, params as P
from tests import variants_cases as vc
from tests.frame_info import newest_info as newest


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = vc.block("linear", iq=True)
    one = lib.beamform(acq.bp, acq.rf, acq.filters)            # the ring's first frame: offset 0
    first = newest(L)
    frame_bytes, base = int(first.size_bytes), int(first.device_pointer)
    n = min(P.HIP_MAX_VARIANTS, ring // frame_bytes * 5 // 8)
    pushes = (ring // frame_bytes - 1) // n                     # runs of n frames that fit behind the single frame
    assert n >= 2 and pushes >= 1 and (pushes + 1) * n + 1 > ring // frame_bytes
    variants = [lib.variant_of(acq.bp, speed_of_sound=1400.0 + 5.0 * k) for k in range(n)]
    runs = []
    for k in range(pushes):
        runs.append(lib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy())
        assert int(newest(L).device_pointer) == base + (k + 1) * n * frame_bytes      # behind what came before, contiguous
    wrapped = lib.beamform_variants(acq.bp, acq.rf, variants, acq.filters).copy()
    assert int(newest(L).device_pointer) == base + (n - 1) * frame_bytes            # the whole run went back to offset 0
    assert np.array_equal(wrapped.view(np.uint32), runs[0].view(np.uint32))
    assert not np.array_equal(wrapped[0], wrapped[1]) and wrapped.shape[1:] == one.shape
    # a run the ring cannot hold is refused and takes no frame id
    bp = type(acq.bp).from_buffer_copy(acq.bp)
    bp.output_points[:3] = [256, 1, 256]                       # 512 KiB a frame: two fit, three do not
    one_big = lib.beamform_variants(bp, acq.rf, variants[:2], acq.filters)
    before = newest(L).frame_id
    array = (P.HipDasVariant * 3)(*variants[:3])
    rf = np.ascontiguousarray(acq.rf)
    assert not L.beamformer_hip_push_data_variants_with_compute(rf.ctypes.data_as(C.c_void_p), rf.nbytes, array, 3, 0, 0)
    assert lib.last_error()[0] == P.LibError.FrameSizeOverflow
    assert newest(L).frame_id == before and one_big.shape == (2, 256, 1, 256)
    print(f"wrapped: {pushes + 1} runs of {n} frames of {frame_bytes} bytes in a ring of {ring}")


if __name__ == "__main__":
    main()
