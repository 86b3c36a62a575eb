"""The scaffolding test modules share: the fixtures that leave the automatic DAS path behind (on the device, and on the host), the
two-contexts-on-one-device dance of the test_several_devices_are_refused tests, and the launcher of the *_wrap_worker.py processes.
Imports nothing of tests/."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def automatic_path(bflib):
    """autouse in every module that imports it by name; a module with teardown of its own wraps it in a fixture that asks for it"""
    L = bflib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    L.beamformer_hip_set_das_path(0)
    yield
    L.beamformer_hip_set_das_path(0)


@pytest.fixture(autouse=True)
def automatic_path_on_the_host():
    """automatic_path for the modules that need no device: no bflib, no timeout; autouse in every module that imports it by name"""
    from ogl_beamforming_amd import lib
    lib.library().beamformer_hip_set_das_path(0)
    yield
    lib.library().beamformer_hip_set_das_path(0)


@contextlib.contextmanager
def two_contexts_on_device_0(bflib, acq):
    """the devices of beamformer_hip_set_devices are ordinal 0 twice (how a one-GPU box tests the path) and one push of `acq` has been
    served by both: yields that frame; a single device again on every way out"""
    L = bflib.library()
    try:
        L.beamformer_hip_shutdown()
        assert L.beamformer_hip_set_devices((C.c_int32 * 2)(0, 0), 2)
        frame = bflib.beamform(acq.bp, acq.rf, acq.filters)
        assert L.beamformer_hip_get_device_count() == 2
        yield frame
    finally:
        L.beamformer_hip_shutdown()
        assert L.beamformer_hip_set_devices((C.c_int32 * 1)(0), 1)


def run_ring_worker(module, ring_bytes, expect, timeout=300, args=()):
    """python -m tests.<module> <args> in a process of its own with a frame ring of `ring_bytes` (the ring is sized once per process): it
    has to end well and say every word of `expect`"""
    env = dict(os.environ, BEAMFORMER_HIP_FRAME_RING_BYTES=str(ring_bytes))
    run = subprocess.run([sys.executable, "-m", "tests." + module, *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert all(word in run.stdout for word in expect), run.stdout
