"""What a progressive step costs, in ONE process and alternating (settings
compared in one process share its shading-time mode): C3 (1024 x 1024, the
GPU-built tree, forward accumulation) at 512 spp as

    one shot | one step of 512 | 8 steps of 64 | 64 steps of 8

one warm-up round and then --frames rounds, each round running the four in that order. Times
are the library's HIP-event device times (izpi_render_stats.total_ms; a session's is the sum
over its steps and does not include snapshots). Then k_resolve alone: snapshots of a 1-spp
session into device memory at 1024 x 1024 and 2048 x 2048 (C5's size), IZPI_SNAP_CANVAS and
IZPI_SNAP_DISPLAY, Colour and Spectral, as the host's wall time around
izpi_gpu_progressive_snapshot_device (tile-list copy, launch and stream synchronise
included: an upper bound of the kernel's time). Written to profiles/<name>/progressive_c3.json.

    python tools/progressive_probe.py --name r9a

Checked here (exit status 1 otherwise): the single step of 512 renders the one shot's samples
through the same kernels without the division and scatter, so its median device time may
exceed the one shot's median by no more than the one shot's own spread (max - min) in this
run. The smaller steps are recorded, not judged: every step drains the wavefront once.
"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, ".")
from izpi_amd import configs
from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer

ap = argparse.ArgumentParser()
ap.add_argument("--name", required=True, help="profiles/<name>/progressive_c3.json")
ap.add_argument("--config", default="C3")
ap.add_argument("--spp", type=int, default=512)
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--snapshots", type=int, default=20, help="timed snapshots per form and size")
a = ap.parse_args()
cfg = configs.configs()[a.config]
r = GPURenderer(cfg.build(), cfg.width, cfg.height, a.spp, max_depth=cfg.max_depth, sampler=cfg.sampler, device=0,
                bvh="gpu", accumulation=N.ACC_FORWARD)
STEPS = {"one_shot": None, "steps_1": a.spp, "steps_8": a.spp // 8, "steps_64": a.spp // 64}
frames = {k: [] for k in STEPS}


def row(st, wall_ms, steps):
    return {"device_ms": round(st["total_ms"], 3), "wall_ms": round(wall_ms, 3), "trace_ms": round(st["kernel_ms"], 3),
            "shade_ms": round(st["shade_ms"], 3), "tail_ms": round(st["tail_ms"], 3), "launches": st["launches"],
            "steps": steps, "rays": st["rays"], "samples": st["samples"], "slots": st["slots"], "chunk_spp": st["chunk_spp"],
            "workspace_gb": round(st["workspace_bytes"] / 1e9, 2)}


for rnd in range(a.warmup + a.frames):
    for name, step in STEPS.items():
        t0 = time.perf_counter()
        if step is None:
            r.render()
            st, steps = r.stats, 0
        else:
            with r.progressive(step) as s:
                steps = 0
                while s.done < s.total:
                    s.step()
                    steps += 1
                st = s.stats
        wall_ms = (time.perf_counter() - t0) * 1e3
        if rnd >= a.warmup:
            frames[name].append(row(st, wall_ms, steps))
        print("probe: round %d %s %.1f ms device" % (rnd, name, st["total_ms"]), file=sys.stderr, flush=True)
r.close()
rays = {f["rays"] for v in frames.values() for f in v}
assert len(rays) == 1, rays  # every split traces the same rays

# ---- k_resolve alone
import torch
resolve = {}
for label, scene, sampler in (("colour", configs.cornell_rgb(), N.SAMPLER_COLOUR),
                              ("spectral", configs.cornell_glass_spectral(), N.SAMPLER_SPECTRAL)):
    for size in (1024, 2048):
        q = GPURenderer(scene, size, size, 1, sampler=sampler, device=0, accumulation=N.ACC_FORWARD)
        out = torch.zeros((size, size, 4), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        with q.progressive(1) as s:
            s.step()
            for form, fname in ((N.SNAP_CANVAS, "canvas"), (N.SNAP_DISPLAY, "display")):
                us = []
                for k in range(3 + a.snapshots):
                    t0 = time.perf_counter()
                    s.snapshot_device(out.data_ptr(), form)
                    if k >= 3:
                        us.append((time.perf_counter() - t0) * 1e6)
                resolve["%s_%s_%d" % (label, fname, size)] = {
                    "median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
                    "bytes": size * size * 56, "gb_per_s_at_min": round(size * size * 56 / min(us) / 1e3, 1)}
        q.close()

med = {k: statistics.median(f["device_ms"] for f in v) for k, v in frames.items()}
spread = max(f["device_ms"] for f in frames["one_shot"]) - min(f["device_ms"] for f in frames["one_shot"])
out = {"config": cfg.name, "width": cfg.width, "height": cfg.height, "spp": a.spp, "bvh": "gpu", "accumulation": "forward",
       "frames": frames, "median_device_ms": med, "one_shot_spread_ms": round(spread, 3),
       "median_wall_ms": {k: statistics.median(f["wall_ms"] for f in v) for k, v in frames.items()},
       "resolve_wall": resolve}
path = Path("profiles") / a.name / "progressive_c3.json"
path.parent.mkdir(parents=True, exist_ok=True)
path.write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps({"median_device_ms": med, "one_shot_spread_ms": round(spread, 3), "resolve_wall": resolve}))
if med["steps_1"] > med["one_shot"] + spread:
    sys.exit("one step of %d: %.3f ms, over the one shot's %.3f ms + its spread %.3f ms"
             % (a.spp, med["steps_1"], med["one_shot"], spread))
