#!/usr/bin/env python3
"""Time the variance-guided denoiser beside the fixed-sigma one.

C3 (the Cornell box with the dragon) at 1024 x 1024 on the GPU-built tree, one process: the
Normal and Albedo guides at 4 spp, then a noise session of --steps steps of --step-spp samples,
whose CANVAS and NOISE snapshots go into device canvases. Then izpi_gpu_denoise_device and
izpi_gpu_denoise_var_device, each at its defaults, alternate on the one context: one warm-up
call and --runs timed calls each (HIP-event time over the iterations; the new entry's includes
k_dnv_init). The figure to read is the ratio of the two medians of this one run: times of
different boxes, or of different processes, do not compare. A second, fresh process repeats
one call of each under `rocprofv3 --kernel-trace --stats`, a run of its own, for the
per-iteration split and k_dnv_init's time. Nothing is judged: the filter has no predecessor.

    python tools/denoise_var_probe.py --out profiles/<round>/denoise_var_probe.json
"""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from izpi_amd import _native as N  # noqa: E402
from izpi_amd import configs  # noqa: E402
from izpi_amd.renderer import GPURenderer, denoise_var_device  # noqa: E402


def spread(values):
    v = sorted(values)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4), "runs": len(v)}


def frames(a):
    """(renderer, {name: device canvas}, session ms): the guides, then the session's two snapshots."""
    import torch
    cfg = configs.configs()[a.config]
    r = GPURenderer(cfg.build(), a.size, a.size, a.steps * a.step_spp, max_depth=cfg.max_depth, sampler=N.SAMPLER_COLOUR,
                    device=a.device, bvh="gpu", accumulation=N.ACC_FORWARD)
    dev = torch.device("cuda", a.device)
    shape = (a.size, a.size, 4)
    t = {name: torch.zeros(shape, dtype=torch.float64, device=dev) for name in ("colour", "stderr", "out", "out_var")}
    t["variance"] = torch.zeros(shape[:2], dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    t["normal"], t["albedo"] = r.render_guides(a.aov_spp)
    session_ms = 0.0
    with r.progressive(a.step_spp, noise=True) as s:
        for _ in range(a.steps):
            s.step()
            session_ms = s.stats["total_ms"]
        s.snapshot_device(t["colour"].data_ptr(), N.SNAP_CANVAS)
        s.snapshot_device(t["stderr"].data_ptr(), N.SNAP_NOISE)
        noise = s.noise()
    return r, t, round(session_ms, 3), noise


def fixed(r, t):
    return r.denoise_device(t["colour"].data_ptr(), t["normal"].data_ptr(), t["albedo"].data_ptr(), t["out"].data_ptr())


def guided(r, t):
    return denoise_var_device(r.ctx, t["colour"].data_ptr(), t["stderr"].data_ptr(), t["normal"].data_ptr(),
                              t["albedo"].data_ptr(), t["out_var"].data_ptr(), t["variance"].data_ptr(), r.width, r.height)


def child(a):
    r, t, _, _ = frames(a)
    for _ in range(2):  # the warm-up calls, then the ones the trace is read for
        fixed(r, t)
        guided(r, t)
    r.close()


def per_iteration(a):
    """Durations (ms) of the last call's launches of each filter, from a kernel trace of a fresh process."""
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, str(Path(__file__).resolve()), "--child", "--config", a.config, "--size", str(a.size),
               "--steps", str(a.steps), "--step-spp", str(a.step_spp), "--aov-spp", str(a.aov_spp), "--device", str(a.device)]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise SystemExit("denoise_var_probe: the traced run failed (status %d)\n%s" % (run.returncode, run.stderr[-2000:]))
        rows = []
        for p in Path(d).rglob("*kernel_trace.csv"):
            with open(p, newline="") as f:
                rows += list(csv.DictReader(f))
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    n = N.DENOISE_DEFAULT_ITERATIONS
    out = {}
    for key, count in (("k_denoise", n), ("k_dnv", n), ("k_dnv_init", 1)):
        mine = [row for row in rows if key in row["Kernel_Name"] and (key != "k_dnv" or "k_dnv_init" not in row["Kernel_Name"])]
        if len(mine) != 2 * count:
            raise SystemExit("denoise_var_probe: expected %d %s launches in the trace, found %d" % (2 * count, key, len(mine)))
        out[key] = [round((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6, 4) for row in mine[count:]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--aov-spp", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tmp", default=None, help="where the traced run's files go for its duration")
    ap.add_argument("--child", action="store_true", help="(the traced run)")
    ap.add_argument("--no-trace", action="store_true", help="leave the traced run out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_var_probe: no HIP device (this measurement needs the GPU)")
    r, t, session_ms, noise = frames(a)
    fixed(r, t)
    guided(r, t)  # warm-up
    times = {"fixed": [], "guided": []}
    for _ in range(a.runs):
        times["fixed"].append(fixed(r, t))
        times["guided"].append(guided(r, t))
    colour, out = t["colour"].cpu().numpy(), t["out_var"].cpu().numpy()
    var = t["variance"].cpu().numpy()
    live = colour[..., 3] != 0
    if not (out[..., 3] == colour[..., 3]).all() or not (out[live] == out[live]).all() or (out[live] == colour[live]).all():
        raise SystemExit("denoise_var_probe: the output is not a filtered copy of the frame")
    r.close()

    res = {
        "config": a.config, "width": a.size, "height": a.size, "session": "%d x %d spp" % (a.steps, a.step_spp),
        "aov_spp": a.aov_spp, "live_pixels": int(live.sum()), "iterations": N.DENOISE_DEFAULT_ITERATIONS,
        "session_total_ms": session_ms, "noise": {k: noise[k] for k in ("pixels", "nonfinite", "above", "max_error", "converged")},
        "sigmas_fixed": [N.DENOISE_DEFAULT_SIGMA_COLOUR, N.DENOISE_DEFAULT_SIGMA_NORMAL, N.DENOISE_DEFAULT_SIGMA_ALBEDO],
        "sigmas_guided": [N.DENOISE_VAR_DEFAULT_SIGMA_COLOUR, N.DENOISE_DEFAULT_SIGMA_NORMAL, N.DENOISE_DEFAULT_SIGMA_ALBEDO],
        "variance_floor": N.DENOISE_VAR_DEFAULT_FLOOR,
        "mean_variance_in": float((t["stderr"].cpu().numpy()[..., :3] ** 2).sum(axis=2)[live].mean()),
        "mean_variance_out": float(var[live].mean()),
        "denoise_device_ms": spread(times["fixed"]),
        "denoise_var_device_ms": spread(times["guided"]),
    }
    res["ratio_of_medians"] = round(res["denoise_var_device_ms"]["median"] / res["denoise_device_ms"]["median"], 4)
    if not a.no_trace:
        res["per_launch_ms_kernel_trace"] = per_iteration(a)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
