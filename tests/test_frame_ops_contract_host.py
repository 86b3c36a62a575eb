"""What every frame operation owes its caller, on the CPU, asked of the operations of tests/frame_ops_table.py: the table holds every
declared operation that takes the ensemble or the produce path of csrc/frame_ops.cpp, once; the count is judged first; and whatever can be decided without a device is refused with
its error kind, leaves the outputs alone and starts no device.  What is about one operation alone -- its limits, its own arguments
-- is in that operation's own *_host.py module."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests.frame_ops_table import IDS, OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError


ENTRY = {"newest_ensemble_frames": "ensemble", "frames_once_a_box": "ensemble", "queue_frames_of_newest": "produce"}


def test_the_table_holds_every_operation_that_takes_the_ensemble_or_the_produce_path():
    """read from the library's source, not from a list: every function of csrc/frame_ops.cpp that the header declares and that calls
    newest_ensemble_frames, frames_once_a_box or queue_frames_of_newest in its own body is the symbol of exactly one record, of that
    family -- a new operation that calls one of these cannot be added without joining the table.  Direct callers only: a call that
    reaches them through a helper of its own (the two map producers through queue_deposit_map) is not seen, and is no part of the
    table"""
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    source = open(os.path.join(ROOT, "ogl_beamforming_amd", "csrc", "frame_ops.cpp")).read()
    declared = set(re.findall(r"BEAMFORMER_LIB_EXPORT \w+ (beamformer_hip_\w+)\(", header))
    found = {}
    for function in re.finditer(r"^bool (\w+)\(.*?^}", source, re.S | re.M):
        symbol, body = "beamformer_hip_" + function.group(1), function.group(0).split("{", 1)[1]
        for entry, family in ENTRY.items():
            if symbol in declared and entry + "(" in body:
                found[symbol] = family
    table = {op.symbol: op.family for op in OPS}
    assert len(table) == len(OPS)
    assert not set(found) - set(table), f"on a shared path and in no record: {sorted(set(found) - set(table))}"
    assert table == found
    for op in OPS:
        assert op.symbol in lib.exported_symbols() and callable(op.helper)


@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_what_needs_no_device_is_refused_and_starts_none(op):
    L = lib.library()
    L.beamformer_hip_shutdown()                       # (no device in use from here on: none of the calls below starts one)

    def refused(kind, count, **change):
        call, untouched = op.bare(count, **change)
        assert not call(L)
        assert lib.last_error()[0] == kind and untouched(), (count, change)

    # BufferOverflow on the count is decided first: before a null output is, before the operation's own arguments are
    for count in (0, op.count_cap + 1, 0xFFFFFFFF):
        refused(E.BufferOverflow, count, sized=2)
        refused(E.BufferOverflow, count, sized=2, null=True)
        for row in op.malformed:
            refused(E.BufferOverflow, count, **dict(row.change(), sized=row.K))
    refused(E.InvalidAccess, 2, null=True)
    for row in op.malformed:
        if row.host:
            refused(row.error, row.K, **row.change())
    # every argument good: no device yet, so there is no frame
    for form in op.forms(2):
        refused(E.InvalidAccess, 2, **form)
    with pytest.raises(lib.BeamformerError):
        op.run(2, np.random.default_rng(1)).call() if op.run else op.plain(2)
    assert not L.beamformer_hip_get_last_frame_info(C.byref(P.HipFrameInfo()))
