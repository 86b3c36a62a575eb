"""The newest frame's record, for the frame-operation tests and for their worker processes (which import nothing heavier)."""
import ctypes as C

from ogl_beamforming_amd import params as P


def newest_info(L):
    info = P.HipFrameInfo()
    assert L.beamformer_hip_get_last_frame_info(C.byref(info))
    return info


def newest_id(L):
    """the newest frame's id; None while the newest push is a tombstone"""
    info = P.HipFrameInfo()
    return int(info.frame_id) if L.beamformer_hip_get_last_frame_info(C.byref(info)) else None
