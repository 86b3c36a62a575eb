"""The DAS selection (csrc/das_select.cpp) decides what it decided: tests/select_digest.cpp runs every entry point of das_select.h over a
fixed lattice of parameter blocks, das path modes and hooks, and prints one line per run -- the run's id, the path of every part, the
part count and a 64-bit hash of every field of every decision.  The lines must equal tests/golden/das_select_digest.txt, and the lattice
must reach every kernel, gate and declining reason of the program's coverage table (its exit status).  No device, no library: host
arithmetic compiled for the host.

After a DELIBERATE change of a rule: `select_digest --full` before and after shows which runs moved and in what; then record the golden
file anew (`select_digest > tests/golden/das_select_digest.txt`)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ogl_beamforming_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "das_select_digest.txt")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    include = next((d for d in ("/opt/rocm/include", "/usr/include") if os.path.exists(os.path.join(d, "hip", "hip_runtime_api.h"))), None)
    if include is None:
        pytest.skip("HIP headers not found")
    exe = tmp_path_factory.mktemp("select_digest") / "select_digest"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I", CSRC,
                            os.path.join(ROOT, "tests", "select_digest.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    return str(exe)


def test_the_lattice_reaches_every_kernel_gate_and_reason(program):
    run = subprocess.run([program, "--coverage"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    table = [line for line in run.stdout.splitlines() if line.startswith("#")]
    required = [line for line in table if "(not required)" not in line]
    assert len(required) >= 36 and all(int(line.split()[-1]) > 0 for line in required), "\n".join(table)


def test_every_decision_is_the_recorded_one(program):
    run = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got, want = run.stdout.splitlines(), open(GOLDEN).read().splitlines()
    moved = [f"{g}   (recorded: {w})" for g, w in zip(got, want) if g != w]
    assert not moved and len(got) == len(want), f"{len(moved)} of {len(want)} runs moved ({len(got)} printed):\n" + "\n".join(moved[:20])
