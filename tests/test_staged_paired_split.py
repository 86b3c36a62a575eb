"""The ONE split of the channel-paired staged kernel's transmits into staging groups (csrc/bf_kernels.h bf_staged_paired_split): the
plan (das_select.cpp), the launcher and the kernel (das_staged.hip) all call it, so they cannot disagree -- checked here on the source
and, for the plan, through beamformer_hip_describe_das (no device needed).  The helper itself is compiled for the host
(tests/paired_split.cpp) and held to what the kernel rests on, for every padded transmit count from 4 to 2 x
BF_STAGED_PAIRED_GROUP_MAX: at most two groups of at most the group maximum, multiples of 4, every transmit in exactly one group (group 0
is transmits 0 .. g0 - 1, group 1 the rest), every window element of a group below the 4096 elements the 16-bit shift of the tap address
reaches, the LDS within half a CU, and no split with fewer staging passes among those that fit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ogl_beamforming_amd", "csrc")
GROUP_MAX, BUDGET = 60, 80 * 1024
CHUNKS = (2, 8, 16, 32, 33, 64)


def lds_bytes(group, chunk, a4):
    """the kernel's LDS layout (das_staged.hip staged_paired_body), restated"""
    return (16 * (group * 64 + 3) + 16 * (((chunk + 1) & ~1) << 5) + 4 * (a4 + 2 * (chunk + 2)) + 128 + 15) & ~15


def passes(group):
    return max(2, -(-group // 16))          # 1024 threads stage 16 transmits' blocks per pass; one pass runs as two


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("paired_split") / "paired_split"
    include = next((d for d in ("/opt/rocm/include", "/usr/include") if os.path.exists(os.path.join(d, "hip", "hip_runtime_api.h"))), None)
    if include is None:
        pytest.skip("HIP headers not found")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I", CSRC,
                            os.path.join(ROOT, "tests", "paired_split.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe), *map(str, CHUNKS)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0
    lines = run.stdout.strip().splitlines()
    assert lines[-1].split() == ["max", str(GROUP_MAX), "budget", str(BUDGET)]
    return {(a4, chunk): (bool(ok), g0, g1, p0, p1, lds) for a4, chunk, ok, g0, g1, p0, p1, lds in
            (tuple(int(v) for v in line.split()) for line in lines[:-1])}


def test_split_invariants_for_every_padded_transmit_count(table):
    assert GROUP_MAX * 64 + 2 < 4096
    for (a4, chunk), (ok, g0, g1, p0, p1, lds) in sorted(table.items()):
        fits = [g for g in range(4, GROUP_MAX + 1, 4) if lds_bytes(g, chunk, a4) <= BUDGET]
        gmax = max(fits) if fits else 0
        splits = ([(a4, 0)] if a4 <= gmax else []) + [(f, a4 - f) for f in range(4, gmax + 1, 4) if 0 < a4 - f <= f]
        assert ok == bool(splits), (a4, chunk)
        if not ok:
            assert a4 > 2 * gmax                                   # refused only where two groups cannot hold the transmits
            continue
        assert g0 + g1 == a4 and g0 % 4 == 0 and g1 % 4 == 0        # [0, g0) and [g0, a4): every transmit exactly once
        assert 0 <= g1 <= g0 <= GROUP_MAX
        for g in (g0, g1):                                          # the last tap element of a group: 2 in front + (g - 1) blocks + 63
            assert 2 + (g - 1) * 64 + 63 < 4096 if g else True
        assert lds == lds_bytes(g0, chunk, a4) <= BUDGET            # two blocks per CU (160 KB)
        assert (p0, p1) == (passes(g0), passes(g1) if g1 else 0)
        cost = lambda s: passes(s[0]) + (passes(s[1]) if s[1] else 0)
        assert cost((g0, g1)) == min(cost(s) for s in splits), (a4, chunk, g0, g1)
    for a4 in range(4, 2 * GROUP_MAX + 1, 4):                       # config 4's chunk of 16 channels takes every count up to 2 x 60
        assert table[(a4, 16)][0], a4
    assert table[(76, 16)][1:3] == (48, 28)                         # config 4: 3 + 2 passes where halves of 40 + 36 were 3 + 3
    assert table[(64, 16)][1:3] == (32, 32) and table[(40, 16)][1:3] == (40, 0) and table[(68, 16)][1:3] == (48, 20)
    assert not table[(124, 16)][0]


def strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_plan_launcher_and_kernel_ask_the_one_helper():
    staged = strip_comments(open(os.path.join(CSRC, "das_staged.hip")).read())
    select = strip_comments(open(os.path.join(CSRC, "das_select.cpp")).read())
    header = strip_comments(open(os.path.join(CSRC, "bf_kernels.h")).read())
    body = staged[staged.index("void staged_paired_body"):staged.index("void das_rca_staged_kernel")]
    launcher = staged[staged.index("launch_staged_shape(const BfDasArgs"):staged.index("bf_launch_das_staged(const BfDasArgs")]
    assert body.count("bf_staged_paired_split(") == 1 and launcher.count("bf_staged_paired_split(") == 1
    assert select.count("bf_staged_paired_split(") == 1 and header.count("bf_staged_paired_split(") == 1
    for text in (staged, select):                                   # no second rule beside it
        assert "BF_STAGED_PAIRED_GROUP_MAX" not in text


@pytest.mark.parametrize("transmits", [5, 40, 44, 60, 61, 64, 67, 75, 80, 85, 100, 117, 120])
def test_the_plan_sizes_its_lds_for_the_helpers_groups(transmits, table):
    """the plan's LDS bytes are those of the helper's larger group for the chunk the plan chose"""
    acq = cfg.rca(f"split{transmits}", 32, transmits, 512, (150, 36, 2), cases.LO3, cases.HI3, seed=70, orientation=0x12, cw=True,
                  f_number=0.6, angles=np.linspace(-12, 12, transmits))
    L = lib.library()
    lib.set_hook("STAGED_SHAPE", "5,5,5")
    L.beamformer_hip_set_das_path(3)
    try:
        d = lib.describe_das(acq.bp, acq.filters)[4]
    finally:
        L.beamformer_hip_set_das_path(0)
        lib.set_hook("STAGED_SHAPE", None)
    assert d.uniform_tables == 2, transmits
    a4, chunk = (transmits + 3) // 4 * 4, int(d.channel_chunk)
    if (a4, chunk) not in table:
        pytest.fail(f"the plan chose a chunk of {chunk} channels: add it to CHUNKS")
    ok, g0, g1 = table[(a4, chunk)][:3]
    assert ok and int(d.lds_bytes) == lds_bytes(g0, chunk, a4) <= BUDGET
