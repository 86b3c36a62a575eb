#!/usr/bin/env python3
"""compare_code_objects.py -- two builds of the library, kernel by kernel: which kernels disassemble to the same instructions
(llvm-objdump -d of the gfx950 code objects, addresses and branch-target labels aside) and, for those that do not, the register /
spill / scratch / LDS figures of both (tools/kernel_resources.py).  The check a refactor of kernel sources runs against its parent:

    python3 tools/compare_code_objects.py build/variants/libogl_parent.so ogl_beamforming_amd/libogl_beamformer_lib.so \\
        --require-identical 'das_rca_staged_kernel<.*, true>' --json profiles/staged_shared_resources.json
"""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, MAGIC, kernels_of


def demangle(names):
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            return subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.strip().split("\n")
        except (OSError, subprocess.CalledProcessError):
            continue
    return names

FIGURES = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def disassembly_of(library):
    """{mangled kernel name: (sha256 of its instruction text, instruction count)}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", library, os.path.join(tmp, "copy.so")], check=True)
        data = open(fat, "rb").read()
        for bi, m in enumerate(re.finditer(re.escape(MAGIC), data)):
            p = m.start()
            off = p + len(MAGIC)
            (count,) = struct.unpack_from("<Q", data, off)
            off += 8
            for _ in range(count):
                o, size, tlen = struct.unpack_from("<QQQ", data, off)
                off += 24
                triple = data[off:off + tlen].decode()
                off += tlen
                if "gfx950" not in triple or size == 0:
                    continue
                co = os.path.join(tmp, f"co_{bi}.o")
                open(co, "wb").write(data[p + o:p + o + size])
                text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                      capture_output=True, text=True, check=True).stdout
                name, lines = None, []
                for line in text.split("\n") + ["<end>:"]:
                    label = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line.strip())
                    if label and not label.group(1).startswith("L"):
                        if name:
                            out[name] = (hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines))
                        name, lines = label.group(1), []
                    elif name and line.strip() and not label:
                        lines.append(re.sub(r"\s*//.*$", "", line.strip()))      # (the comment column holds the address)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("library")
    ap.add_argument("--require-identical", action="append", default=[], help="regex on the demangled name: these kernels must disassemble alike")
    ap.add_argument("--edited", default=r"das_rca_staged_kernel<|das_rca_staged_real_kernel<|das_rca_staged_cubic_kernel<|das_rca_separable_kernel<|staged_tables_kernel<",
                    help="regex on the demangled name: kernels of the edited files (every other kernel must disassemble alike)")
    ap.add_argument("--json")
    args = ap.parse_args()
    dis = [disassembly_of(args.parent), disassembly_of(args.library)]
    res = [{k["name"]: k for k in kernels_of(lib)} for lib in (args.parent, args.library)]
    names = sorted(set(dis[0]) | set(dis[1]))
    pretty = dict(zip(names, demangle(names)))
    identical, differing, failures = [], [], []
    for n in names:
        d = re.sub(r"\(anonymous namespace\)::", "", pretty[n])
        d = re.sub(r"^void ", "", d).split("(")[0]
        if n not in dis[0] or n not in dis[1]:
            failures.append(f"only in one library: {d}")
            continue
        same = dis[0][n][0] == dis[1][n][0]
        must = any(re.search(r, d) for r in args.require_identical) or not re.search(args.edited, d)
        if same:
            identical.append(d)
            continue
        if must:
            failures.append(f"disassembly differs: {d}")
        a, b = res[0][n], res[1][n]
        row = {"kernel": d, "instructions": [dis[0][n][1], dis[1][n][1]]}
        for f in FIGURES:
            row[f] = [a[f], b[f]]
        differing.append(row)
        if b["vgpr_count"] > a["vgpr_count"]:
            failures.append(f"vgpr_count rose: {d}")
        if b["vgpr_spill_count"] or b["private_segment_fixed_size"]:
            failures.append(f"vector spills or scratch: {d}")
        if a["group_segment_fixed_size"] != b["group_segment_fixed_size"]:
            failures.append(f"group_segment_fixed_size changed: {d}")
    families = {}
    for row in differing:
        fam = families.setdefault(row["kernel"].split("<")[0], {"kernels": 0, "sgpr_spills": [0, 0], "instructions": [0, 0], "sgpr_spills_rose": []})
        fam["kernels"] += 1
        for i in (0, 1):
            fam["sgpr_spills"][i] += row["sgpr_spill_count"][i]
            fam["instructions"][i] += row["instructions"][i]
        if row["sgpr_spill_count"][1] > row["sgpr_spill_count"][0]:
            fam["sgpr_spills_rose"].append(row["kernel"])
    for name, fam in families.items():
        if fam["sgpr_spills"][1] > fam["sgpr_spills"][0]:
            failures.append(f"sum of scalar spills rose: {name} {fam['sgpr_spills']}")
    summary = {"columns": "[parent, this build]", "kernels": len(names), "identical_disassembly": len(identical),
               "required_identical": args.require_identical + ["every kernel not matching: " + args.edited],
               "identical_among_required": sorted(d for d in identical if any(re.search(r, d) for r in args.require_identical)),
               "failures": failures, "families_that_differ": families, "kernels_that_differ": differing}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(f"{len(names)} kernels, {len(identical)} identical, {len(differing)} differ, {len(failures)} failures")
    for name, fam in sorted(families.items()):
        print("  ", name, {k: v for k, v in fam.items() if k != "sgpr_spills_rose"}, "rose in", len(fam["sgpr_spills_rose"]))
    for f in failures:
        print("FAIL", f)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
