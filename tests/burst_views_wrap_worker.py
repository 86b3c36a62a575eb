"""Child process of tests/test_gpu_burst_views.py: burst views pushes in a frame ring of BEAMFORMER_HIP_FRAME_RING_BYTES (the ring is
sized once per process).  A run of N x K frames that would straddle the end of the ring starts again at offset 0, contiguous and
view-major, and stays exportable; a run the ring cannot hold is refused whole.
Started as python -m tests.burst_views_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
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
    lib.beamform(acq.bp, acq.rf, acq.filters)                  # the ring's first frame: offset 0
    first = newest(L)
    own_bytes, base = int(first.size_bytes), int(first.device_pointer)
    patch = lib.view((16, 1, 16), (-4e-3, 0, 10e-3), (-3e-3, 0, 11e-3))
    patch_bytes = own_bytes // int(np.prod(list(acq.bp.output_points[:3]))) * 256
    views = [lib.view_of(acq.bp), patch]
    per_rf = own_bytes + patch_bytes
    n = ring // per_rf * 5 // 8                                 # two such runs do not fit the ring
    assert 5 <= n <= P.HIP_MAX_BURST_FRAMES and 2 * n * per_rf + own_bytes > ring >= n * per_rf + own_bytes
    rng = np.random.default_rng(6)
    rf = np.clip(np.rint(rng.normal(0, 1000.0, (n,) + acq.rf.shape)), -32000, 32000).astype(acq.rf.dtype)
    a = lib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    assert lib.last_burst_views_info().route.rung == 1
    # behind the single frame: n frames of the own grid, then n patches -- the newest frame is the last patch
    assert int(newest(L).device_pointer) == base + own_bytes + n * own_bytes + (n - 1) * patch_bytes
    b = lib.beamform_burst_views(acq.bp, rf, views, acq.filters)
    assert int(newest(L).device_pointer) == base + n * own_bytes + (n - 1) * patch_bytes      # the whole run went back to offset 0
    for v in range(2):
        for k in range(n):
            assert np.array_equal(a[v][k].view(np.uint32), b[v][k].view(np.uint32)), (v, k)
    assert not np.array_equal(a[0][0], a[0][1]) and not np.array_equal(a[1][0], a[1][1])
    # the records the second run overwrote are gone; the newest 2 n are all there
    both = np.zeros(n * per_rf // 4, np.float32)
    assert L.beamformer_get_last_frames(both.ctypes.data_as(C.c_void_p), both.nbytes, 2 * n)
    # a run the ring cannot hold is refused whole and takes no frame id
    before = newest(L).frame_id
    too_many = ring // per_rf + 1
    big = np.zeros((too_many,) + acq.rf.shape, acq.rf.dtype)
    array = (P.HipView * 2)(*views)
    assert not L.beamformer_hip_push_data_burst_views_with_compute(big.ctypes.data_as(C.c_void_p), big[0].nbytes, too_many, array, 2, 0)
    assert lib.last_error()[0] == P.LibError.FrameSizeOverflow
    lib.beamform(acq.bp, acq.rf, acq.filters)
    assert newest(L).frame_id == before + 1
    print(f"wrapped: {n} RF frames on 2 views, {per_rf} bytes a frame pair, twice in a ring of {ring}")


if __name__ == "__main__":
    main()
