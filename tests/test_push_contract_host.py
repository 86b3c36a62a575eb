"""What every multi-frame push owes its caller, on the CPU, asked of all six kinds of tests/push_kinds.py: the entry points exist and
are bound, the kind's DAS kernel is in the library with its instantiations, and a malformed push, a run larger than the frame ring and
a push with several devices asked for are refused before any device is touched (csrc/lib_api.cpp multi_push_ready and the checks in
front of it).  What is about one kind alone -- its describe call's routes, its thresholds -- is in that kind's own *_host.py module."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P
from tests.das_push import push_parameters
from tests.push_kinds import IDS, KINDS, Row, two_devices_asked_for
from tests.scaffold import automatic_path_on_the_host  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = P.LibError


@pytest.fixture(autouse=True)
def two_parameter_blocks(automatic_path_on_the_host):
    """(the READI image's rows push a block that is not READI in a second slot)"""
    L = lib.library()
    L.beamformer_reserve_parameter_blocks(2)
    yield
    L.beamformer_reserve_parameter_blocks(1)


def frames_taken():
    """the id the next push would take, as far as the host knows it: a refused push must leave it where it was.  Without a device
    there is no frame to ask for: the frame info call fails both before and after."""
    info = P.HipFrameInfo()
    ok = lib.library().beamformer_hip_get_last_frame_info(C.byref(info))
    return (ok, int(info.frame_id) if ok else None)


def test_no_kind_is_left_out_of_a_rule_silently():
    """a kind is exempt only with a reason that names the line of the library that makes it so; the tombstones are asked of exactly the
    kinds whose pushes the executor fails on flag 0x2000, on every route: 2 + 3 + 2 ids"""
    for kind in KINDS:
        assert kind.fails_on_flag != ("tombstones" in kind.exempt), kind.name
        assert all("executor.cpp:" in reason or "lib_api.cpp:" in reason for reason in kind.exempt.values()), kind.name
    assert sum(len(kind.routes) for kind in KINDS if kind.fails_on_flag) == 7


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_the_symbols_are_declared_exported_and_bound(kind, tmp_path):
    header = open(os.path.join(ROOT, "include", "ogl_beamformer_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIBRARY_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if " T " in line}
    for name in kind.symbols:
        assert f"{name}(" in header, name
        assert name in exported, name
        assert name in lib.exported_symbols(), name
        assert hasattr(lib.library(), name), name
    for line in kind.header:
        assert line in header, line
    for value, expected in kind.constants:
        assert value == expected, (value, expected)
    for struct, size in kind.sizes:
        assert C.sizeof(struct) == size, struct
    # ... and the header's own sizes and offsets, by the C compiler
    asserts = []
    for name, struct, fields in kind.layout:
        asserts.append(f"_Static_assert(sizeof({name}) == {C.sizeof(struct)}, \"{name}\");\n")
        asserts += [f"_Static_assert(offsetof({name}, {f}) == {getattr(struct, f).offset}, \"{name}.{f}\");\n" for f in fields]
    source = tmp_path / "sizes.c"
    source.write_text('#include <stddef.h>\n#include "ogl_beamformer_hip.h"\n' + "".join(asserts))
    run = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(source)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM binutils")
@pytest.mark.parametrize("kind", [k for k in KINDS if "kernels" not in k.exempt], ids=[k.name for k in KINDS if "kernels" not in k.exempt])
def test_the_kernel_has_its_instantiations_without_spills(kind):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert kind.kernels
    for expected in kind.kernels:
        kernels = [k for k in kernel_resources.kernels_of(lib.LIBRARY_PATH) if expected.pattern in k["demangled"]]
        assert len({k["demangled"] for k in kernels}) == expected.count, sorted(k["demangled"] for k in kernels)
        for k in kernels:
            assert not k["vgpr_spill_count"] and not k["private_segment_fixed_size"], k["demangled"]      # 0 vector spills, 0 scratch
            if expected.no_sgpr_spills:
                assert not k["sgpr_spill_count"], k["demangled"]
            if expected.max_vgprs is not None:
                assert k["vgpr_count"] <= expected.max_vgprs, (k["demangled"], k["vgpr_count"])
            if expected.no_lds:
                assert not k["group_segment_fixed_size"], k["demangled"]


def common_rows(kind):
    """the checks every kind makes: the count, the list where the push needs one, and the single push's checks of the RF frame with
    its error kinds (csrc/lib_api.cpp valid_rf_frame)"""
    rows = [Row(dict(count=0), E.BufferOverflow), Row(dict(count=kind.max_count + 1), E.BufferOverflow)]
    if "null_list" not in kind.exempt:
        rows.append(Row(dict(extra=None), E.InvalidAccess))
    return rows + [Row(dict(size_delta=-2), E.DataSizeMismatch), Row(dict(size_delta=2), E.DataSizeMismatch),
                   Row(dict(slot=5), E.ParameterBlockUnallocated), Row(dict(null_data=True), E.BufferOverflow)]


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_malformed_pushes_are_refused_before_a_device_is_touched(kind, capfd):
    case = kind.case("malformed")
    L = push_parameters(case.acq)
    rf, data, size = kind.data(case)
    before = frames_taken()
    for row in common_rows(kind):
        for device in (False, True):
            assert not kind.raw(L, case, data, size, device=device, **row.overrides) and lib.last_error()[0] == row.error, (row, device)
    capfd.readouterr()
    for row in kind.malformed(case):
        if row.push:
            assert not kind.raw(L, case, data, size, **row.overrides) and lib.last_error()[0] == row.error, row
            assert row.word is None or row.word in capfd.readouterr().err, row
            push_parameters(case.acq)              # (a row may have pushed another block)
        if row.describe:
            assert not kind.describe(L, case, **row.overrides) and lib.last_error()[0] == row.error, row
        capfd.readouterr()
    if kind.whole_grid:
        # an output shard on the block
        try:
            assert L.beamformer_hip_set_output_shard(0, *case.shard)
            assert not kind.raw(L, case, data, size) and lib.last_error()[0] == E.InvalidAccess
            assert "not sharded" in capfd.readouterr().err
        finally:
            assert L.beamformer_hip_set_output_shard(0, 0, 0)
    assert frames_taken() == before


@pytest.mark.parametrize("kind", [k for k in KINDS if "too_large" not in k.exempt], ids=[k.name for k in KINDS if "too_large" not in k.exempt])
def test_a_run_larger_than_the_frame_ring_is_refused_whole(kind):
    rows = kind.too_large()
    assert rows
    for case, overrides, instead in rows:
        if instead is not None:
            instead(case)
            continue
        L = push_parameters(case.acq)
        rf, data, size = kind.data(case)
        assert not kind.raw(L, case, data, size, **overrides) and lib.last_error()[0] == E.FrameSizeOverflow, (case.acq.name, overrides)


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_several_devices_are_refused_before_a_device_is_touched(kind, capfd):
    case = kind.case("devices")
    L = push_parameters(case.acq)
    rf, data, size = kind.data(case)
    with two_devices_asked_for(L):
        capfd.readouterr()
        assert not kind.raw(L, case, data, size)
        assert lib.last_error()[0] == E.InvalidAccess and "one device" in capfd.readouterr().err
