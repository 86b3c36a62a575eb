"""Same-box alternating A/B of two builds of the library over a list of measurement rows: every row is a command that prints JSON
lines; it runs `--runs` times a side, the parent's library first in every pair (OGL_BEAMFORMER_LIB selects it), and one figure is read
from each run.  Records per row both sides' runs, medians, spreads (max - min of a side) and the difference, and applies the project's
bar (profiles/README.md): a row is slower when its median is worse than the parent's by more than three times the parent's spread.
Run from the repository root on a GPU box:
  PYTHONPATH=. python tools/ab_rows.py --parent build/variants/libogl_parent.so --rows headline,gather --json out.json"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

BENCH = [sys.executable, "bench.py", "--gpus", "1", "--config", "4", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"]


def last_json(text, want):
    for line in reversed(text.strip().split("\n")):
        line = line.strip()
        if line.startswith("{") or line.startswith("["):
            try:
                v = json.loads(line)
            except ValueError:
                continue
            if want(v):
                return v
    raise RuntimeError("no JSON result line in:\n" + text[-2000:])


def bench_row(extra):
    def run(env):
        out = subprocess.run(BENCH + extra, env=env, capture_output=True, text=True, check=True, timeout=600).stdout
        v = last_json(out, lambda v: isinstance(v, dict) and "ms_per_step" in v)
        return {"figure": float(v["ms_per_step"]), "das_path": v["config"]["das_path"]}
    return run


def uniform_rows(env):
    out = subprocess.run([sys.executable, "tools/staged_uniform.py", "--scales", "0.5"], env=env, capture_output=True, text=True, check=True, timeout=600).stdout
    v = last_json(out, lambda v: isinstance(v, dict) and "uniform_ms" in v)
    return {"figure": float(v["uniform_ms"]), "das_path": v["uniform_path"], "tables_in_lds_ms": float(v["tables_in_lds_ms"]), "tables_in_lds_path": v["tables_in_lds_path"]}


def real_row(env):
    out = subprocess.run([sys.executable, "tools/staged_real_rate.py"], env=env, capture_output=True, text=True, check=True, timeout=600).stdout
    v = last_json(out, lambda v: isinstance(v, dict) and "das_ms_median" in v)
    return {"figure": float(v["das_ms_median"]), "das_path": v["das_path"]}


FIGURE_KEYS = ("_us", "_us_per_frame", "_us_per_push", "_ms")


def medians(value, path, out):
    """the timings a row keeps as {median_us, min_us, max_us} summaries, however deep: one figure each, its median, named by its path"""
    if isinstance(value, dict):
        if isinstance(value.get("median_us"), (int, float)):
            out[path + ".median_us"] = float(value["median_us"])
        for k, v in value.items():
            medians(v, f"{path}.{k}" if path else k, out)


def tool_rows(command):
    """every row a rate tool prints (tools/*_rate.py: one JSON object a row), as one figure per timing of the row -- its keys that end
    in _us, _us_per_frame, _us_per_push or _ms, spreads left out, and the medians of its timing summaries --, named by the row's first
    four plain fields (the case and its counts)"""
    def run(env):
        out = subprocess.run([sys.executable] + command, env=env, capture_output=True, text=True, check=True, timeout=900).stdout
        figures = {}
        for line in out.splitlines():
            if not line.startswith("{"):
                continue
            row = json.loads(line)
            timings = {k: float(v) for k, v in row.items() if k.endswith(FIGURE_KEYS) and "spread" not in k and isinstance(v, (int, float))}
            medians(row, "", timings)
            plain = [f"{k}={v}" for k, v in row.items() if k not in timings and isinstance(v, (str, int)) and not isinstance(v, bool)][:4]
            for k, v in timings.items():
                figures[" ".join(plain + [k])] = v
        assert figures, out[-2000:]
        return {"figures": figures, "das_path": "-"}
    return run


def hostpush_rows(env):
    """tools/hostpush.py: frame time and enqueue time of configs 1-4, device and host pushes"""
    out = subprocess.run([sys.executable, "tools/hostpush.py"], env=env, capture_output=True, text=True, check=True, timeout=900).stdout
    figures = {}
    for cfg, mode, frame, enqueue in re.findall(r"cfg(\d) (\w+)\s+rf .*? frame\s+([\d.]+) us\s+enqueue\s+([\d.]+) us/frame", out):
        figures[f"cfg{cfg} {mode} frame_us"] = float(frame)
        figures[f"cfg{cfg} {mode} enqueue_us"] = float(enqueue)
    assert len(figures) == 16, out[-2000:]
    return {"figures": figures, "das_path": "-"}


ROWS = {
    "headline": ("bench.py config 4 (channel-paired staged kernel: identical code, the noise reference), ms per step", bench_row([])),
    "gather": ("bench.py config 4 --das-path 2 (gather kernel), ms per step", bench_row(["--das-path", "2"])),
    "cubic": ("bench.py config 4 --interpolation cubic (staged cubic kernel), ms per step", bench_row(["--interpolation", "cubic"])),
    "uniform": ("tools/staged_uniform.py --scales 0.5, 32 planes: unpaired complex kernel, uniform tables, DAS ms (tables in LDS beside it)", uniform_rows),
    "real": ("tools/staged_real_rate.py: real-sample staged kernel on config 4's geometry without Demodulate, median DAS ms of 5 pushes", real_row),
    # host time per push: the single push and every multi-frame push, each rate tool at the smallest and largest count of its profile
    "hostpush": ("tools/hostpush.py, us", hostpush_rows),
    "burst_rate": ("tools/burst_rate.py --frames 2,256", tool_rows(["tools/burst_rate.py", "--frames", "2,256"])),
    "views_rate": ("tools/views_rate.py --views 1,256", tool_rows(["tools/views_rate.py", "--views", "1,256"])),
    "readi_rate": ("tools/readi_rate.py --groups 4 --extra-frames 5 (4 to 64 frames)", tool_rows(["tools/readi_rate.py", "--groups", "4", "--extra-frames", "5"])),
    "readi_image_rate": ("tools/readi_image_rate.py --groups 4,16", tool_rows(["tools/readi_image_rate.py", "--groups", "4,16"])),
    "burst_views_rate": ("tools/burst_views_rate.py --frames 2,256", tool_rows(["tools/burst_views_rate.py", "--frames", "2,256"])),
    "variants_rate": ("tools/variants_rate.py --counts 1,64", tool_rows(["tools/variants_rate.py", "--counts", "1,64"])),
    # time per call of the operations on frames already in the ring (csrc/frame_ops.cpp): each rate tool at its smallest and its default counts
    "frame_metrics_rate": ("tools/frame_metrics_rate.py --counts 1,64 --host-repeats 1", tool_rows(["tools/frame_metrics_rate.py", "--counts", "1,64", "--host-repeats", "1"])),
    "frame_peaks_rate": ("tools/frame_peaks_rate.py --counts 1,64 --fractions 0.5,0 --host-repeats 1",
                         tool_rows(["tools/frame_peaks_rate.py", "--counts", "1,64", "--fractions", "0.5,0", "--host-repeats", "1"])),
    "ensemble_filter_rate": ("tools/ensemble_filter_rate.py --plane-counts 8,64 --volume-counts 8,64",
                             tool_rows(["tools/ensemble_filter_rate.py", "--plane-counts", "8,64", "--volume-counts", "8,64"])),
    "autocorr_rate": ("tools/autocorr_rate.py", tool_rows(["tools/autocorr_rate.py"])),
    "spatial_rate": ("tools/spatial_rate.py", tool_rows(["tools/spatial_rate.py"])),
    "motion_rate": ("tools/motion_rate.py", tool_rows(["tools/motion_rate.py"])),
    "warp_rate": ("tools/warp_rate.py", tool_rows(["tools/warp_rate.py"])),
    "localisation_rate": ("tools/localisation_rate.py", tool_rows(["tools/localisation_rate.py"])),
    "frame_quantiles_rate": ("tools/frame_quantiles_rate.py --counts 1,64 --host-repeats 1",
                             tool_rows(["tools/frame_quantiles_rate.py", "--counts", "1,64", "--host-repeats", "1"])),
    "pairs_rate": ("tools/pairs_rate.py", tool_rows(["tools/pairs_rate.py"])),
    "tracks_rate": ("tools/tracks_rate.py", tool_rows(["tools/tracks_rate.py"])),
    "draw_rate": ("tools/draw_rate.py", tool_rows(["tools/draw_rate.py"])),
    "block_filter_rate": ("tools/block_filter_rate.py", tool_rows(["tools/block_filter_rate.py"])),
}


def write_result(path, result):
    """the result as JSON, one row a line (a rate tool's rows are some fifty figures each)"""
    head = {k: v for k, v in result.items() if k != "rows"}
    rows = ",\n".join(f" {json.dumps(name)}: {json.dumps(row)}" for name, row in result["rows"].items())
    with open(path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "rows": {\n' + rows + "\n }\n}\n")


def side(runs, key="figure"):
    vals = [r[key] for r in runs]
    return {"runs": vals, "median": statistics.median(vals), "spread": max(vals) - min(vals)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--library", default=os.path.join("ogl_beamforming_amd", "libogl_beamformer_lib.so"))
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    result = {"what": "same-box alternating A/B, parent first in every pair, lower is better; slower = median over the parent's by more than 3 x the parent's spread",
              "runs_a_side": args.runs, "rows": {}}
    for name in args.rows.split(","):
        what, run = ROWS[name]
        sides = {"parent": [], "this": []}
        for _ in range(args.runs):
            for label, library in (("parent", args.parent), ("this", args.library)):
                env = dict(os.environ, OGL_BEAMFORMER_LIB=os.path.abspath(library), PYTHONPATH=os.getcwd())
                sides[label].append(run(env))
        # a row of several figures is one row per figure
        figures = sorted(sides["parent"][0].get("figures", {}))
        for label in sides:
            sides[label] = [dict(r, **r.get("figures", {})) for r in sides[label]]
        for figure in figures or ["figure"]:
            key = name + ": " + figure if figures else name
            row = {"what": what, "parent": side(sides["parent"], figure), "this": side(sides["this"], figure),
                   "das_path": sorted({str(r["das_path"]) for r in sides["parent"] + sides["this"]})}
            if name == "uniform":
                row["tables_in_lds"] = {"parent": side(sides["parent"], "tables_in_lds_ms"), "this": side(sides["this"], "tables_in_lds_ms")}
                t = row["tables_in_lds"]
                t["difference"] = t["this"]["median"] - t["parent"]["median"]
                t["slower"] = t["difference"] > 3.0 * t["parent"]["spread"]
            row["difference"] = row["this"]["median"] - row["parent"]["median"]
            row["bar"] = 3.0 * row["parent"]["spread"]
            row["slower"] = row["difference"] > row["bar"]
            result["rows"][key] = row
            print(json.dumps({key: {k: row[k] for k in ("parent", "this", "difference", "bar", "slower")}}), flush=True)
        if args.json:
            write_result(args.json, result)
