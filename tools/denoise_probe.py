#!/usr/bin/env python3
"""Time the denoiser on a frame of the size users look at.

C3 (the Cornell box with the dragon) at 1024 x 1024 on the GPU-built tree, one process: the
Colour frame at 16 spp and the Normal and Albedo frames at 4 spp are rendered once into
device canvases, then izpi_gpu_denoise_device runs at the library's defaults, one warm-up
call and --runs timed calls (HIP-event time over the iterations). A second, fresh process
repeats one call under `rocprofv3 --kernel-trace --stats`, a run of its own, for the
per-iteration split. The least time the hardware could take is reported beside it:

  bytes   every iteration reads the colour canvas and both guides and writes one canvas,
          4 x 32 MB, over the HBM peak (the taps re-read lines that the caches hold);
  f64     operations counted from the rule (OPS_PER_TAP below: a division counts as one),
          25 taps per pixel, over the vector FP64 peak.

Peaks are AMD's data-sheet figures for the MI355X: 8 TB/s of HBM3E and 78.6 TFLOP/s of vector
FP64, which counts a fused multiply-add as two; this code is built without contraction, so
it could reach half of that at most. Nothing is judged: the feature has no predecessor.

    python tools/denoise_probe.py --out profiles/<round>/denoise_probe.json
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
from izpi_amd.renderer import GPURenderer  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12
FP64_VECTOR_PEAK_FLOPS = 78.6e12
# f64 operations of one tap with both guides, in the order of denoise.h's pixel():
OPS_PER_TAP = {
    "three squared distances (3 sub, 3 mul, 2 add each)": 24,
    "e = dc*kc + dn*kn + da*ka": 5,
    "gm::exp(-e): reduction 7, polynomial 10, reconstruction 6 (one division), ldexp 1": 24,
    "w = (h*h) * exp": 2,
    "sw += w; sc[k] += w * c[k]": 7,
}
OPS_PER_PIXEL = 25 * sum(OPS_PER_TAP.values()) + 3  # + the three final divisions


def spread(values):
    v = sorted(values)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4), "runs": len(v)}


def frames(a):
    """(renderer, colour, normal, albedo, out) with the three frames rendered, and their device ms."""
    import torch
    cfg = configs.configs()[a.config]
    r = GPURenderer(cfg.build(), a.size, a.size, a.spp, max_depth=cfg.max_depth, sampler=N.SAMPLER_COLOUR,
                    device=a.device, bvh="gpu", accumulation=N.ACC_FORWARD)
    dev = torch.device("cuda", a.device)
    t = [torch.zeros((a.size, a.size, 4), dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize(dev)
    ms = {}
    for name, sampler, spp, canvas in (("colour", N.SAMPLER_COLOUR, a.spp, t[0]), ("normal", N.SAMPLER_NORMAL, a.aov_spp, t[1]),
                                       ("albedo", N.SAMPLER_ALBEDO, a.aov_spp, t[2])):
        r.sampler = sampler
        r.render_device(canvas.data_ptr(), spp=spp)  # the first call of a sampler loads its code
        ms[name] = round(r.render_device(canvas.data_ptr(), spp=spp)["total_ms"], 3)
    r.sampler = N.SAMPLER_COLOUR
    return r, t, ms


def child(a):
    r, t, _ = frames(a)
    for _ in range(2):  # the warm-up call, then the one the trace is read for
        r.denoise_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr())
    r.close()


def per_iteration(a):
    """Durations (ms) of the last call's k_denoise launches, from a kernel trace of a fresh process."""
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, str(Path(__file__).resolve()), "--child", "--config", a.config, "--size", str(a.size),
               "--spp", str(a.spp), "--aov-spp", str(a.aov_spp), "--device", str(a.device)]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise SystemExit("denoise_probe: the traced run failed (status %d)\n%s" % (run.returncode, run.stderr[-2000:]))
        rows = []
        for p in Path(d).rglob("*kernel_trace.csv"):
            with open(p, newline="") as f:
                rows += [row for row in csv.DictReader(f) if "k_denoise" in row["Kernel_Name"]]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    n = N.DENOISE_DEFAULT_ITERATIONS
    if len(rows) != 2 * n:
        raise SystemExit("denoise_probe: expected %d k_denoise launches in the trace, found %d" % (2 * n, len(rows)))
    return [round((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6, 4) for row in rows[n:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--aov-spp", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tmp", default=None, help="where the traced run's files go for its duration")
    ap.add_argument("--child", action="store_true", help="(the traced run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_probe: no HIP device (this measurement needs the GPU)")
    r, t, render_ms = frames(a)
    ptrs = [x.data_ptr() for x in t]
    r.denoise_device(*ptrs)  # warm-up
    timed = [r.denoise_device(*ptrs) for _ in range(a.runs)]
    colour, out = t[0].cpu().numpy(), t[3].cpu().numpy()
    live = colour[..., 3] != 0
    if not (out[..., 3] == colour[..., 3]).all() or not (out[live] == out[live]).all() or (out[live] == colour[live]).all():
        raise SystemExit("denoise_probe: the output is not a filtered copy of the frame")
    r.close()

    pixels = a.size * a.size
    n = N.DENOISE_DEFAULT_ITERATIONS
    bytes_per_iteration = 4 * pixels * 32
    ops_per_iteration = int(live.sum()) * OPS_PER_PIXEL
    floor_bytes_ms = bytes_per_iteration / HBM_PEAK_BYTES_PER_S * 1e3
    floor_ops_ms = ops_per_iteration / FP64_VECTOR_PEAK_FLOPS * 1e3
    res = {
        "config": a.config, "width": a.size, "height": a.size, "colour_spp": a.spp, "aov_spp": a.aov_spp,
        "live_pixels": int(live.sum()), "iterations": n,
        "sigmas": [N.DENOISE_DEFAULT_SIGMA_COLOUR, N.DENOISE_DEFAULT_SIGMA_NORMAL, N.DENOISE_DEFAULT_SIGMA_ALBEDO],
        "render_device_ms": render_ms,
        "denoise_device_ms": spread(timed),
        "per_iteration_ms_kernel_trace": per_iteration(a),
        "least_time": {
            "bytes_per_iteration": bytes_per_iteration, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
            "ms_per_iteration_by_bytes": round(floor_bytes_ms, 5),
            "f64_ops_per_tap": OPS_PER_TAP, "f64_ops_per_pixel": OPS_PER_PIXEL, "f64_ops_per_iteration": ops_per_iteration,
            "fp64_vector_peak_flops": FP64_VECTOR_PEAK_FLOPS, "ms_per_iteration_by_f64_ops": round(floor_ops_ms, 5),
            "bound_by": "f64 operations" if floor_ops_ms > floor_bytes_ms else "bytes",
            "ms_per_call": round(n * max(floor_bytes_ms, floor_ops_ms), 5),
        },
    }
    res["share_of_least_time"] = round(res["least_time"]["ms_per_call"] / res["denoise_device_ms"]["median"], 4)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
