"""Frame times of the preview samplers next to the Colour sampler's, in ONE process and
alternating (settings compared in one process share its shading-time mode):
C3 (1024 x 1024, the GPU-built tree) at 16 spp with Colour forward, Normal, Albedo and
WireFrame, 2 warm-up rounds and then 5 frames each, written with each frame's stats to
profiles/<name>/preview_c3.json.

    python tools/preview_probe.py --name r7a

Normal and Albedo trace the Colour sampler's primary rays and nothing after them: each must
take less time per frame than Colour in the same run (checked here: exit status 1 otherwise).
WireFrame runs two traversals and is only recorded.
"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, ".")
from izpi_amd import configs
from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer

ap = argparse.ArgumentParser()
ap.add_argument("--name", required=True, help="profiles/<name>/preview_c3.json")
ap.add_argument("--config", default="C3")
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--frames", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
cfg = configs.configs()[a.config]
r = GPURenderer(cfg.build(), cfg.width, cfg.height, a.spp, max_depth=cfg.max_depth, sampler=N.SAMPLER_COLOUR, device=0,
                bvh="gpu", accumulation=N.ACC_FORWARD, ink=(1.0, 1.0, 1.0))
samplers = {"colour": N.SAMPLER_COLOUR, "normal": N.SAMPLER_NORMAL, "albedo": N.SAMPLER_ALBEDO, "wireframe": N.SAMPLER_WIREFRAME}
frames = {k: [] for k in samplers}
for rnd in range(a.warmup + a.frames):
    for name, s in samplers.items():
        r.sampler = s
        t0 = time.perf_counter()
        r.render()
        wall_ms = (time.perf_counter() - t0) * 1e3
        if rnd >= a.warmup:
            st = r.stats
            frames[name].append({"wall_ms": round(wall_ms, 3), "device_ms": round(st["total_ms"], 3),
                                 "trace_ms": round(st["kernel_ms"], 3), "shade_ms": round(st["shade_ms"], 3),
                                 "rays": st["rays"], "samples": st["samples"], "node_visits": st["node_visits"],
                                 "tri_tests": st["tri_tests"], "launches": st["launches"],
                                 "workspace_gb": round(st["workspace_bytes"] / 1e9, 2)})
r.close()
out = {"config": cfg.name, "width": cfg.width, "height": cfg.height, "spp": a.spp, "bvh": "gpu", "frames": frames,
       "median_device_ms": {k: statistics.median(f["device_ms"] for f in v) for k, v in frames.items()},
       "median_wall_ms": {k: statistics.median(f["wall_ms"] for f in v) for k, v in frames.items()}}
path = Path("profiles") / a.name / "preview_c3.json"
path.parent.mkdir(parents=True, exist_ok=True)
path.write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps({"median_device_ms": out["median_device_ms"], "median_wall_ms": out["median_wall_ms"]}))
slow = [k for k in ("normal", "albedo") if not max(f["wall_ms"] for f in frames[k]) < min(f["wall_ms"] for f in frames["colour"])]
if slow:
    sys.exit("slower than Colour at the same spp: %s" % ", ".join(slow))
