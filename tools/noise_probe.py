"""What the noise estimate of a progressive session costs, in ONE process and
alternating (settings compared in one process share its shading-time mode):
C3 (1024 x 1024, the GPU-built tree, forward accumulation) as a session of 8 steps of 64
samples,

    plain | with IZPI_PROG_NOISE

one warm-up round and then --rounds rounds, each running the two in that order. The session's
time is the library's HIP-event device time summed over its steps (izpi_render_stats.total_ms:
k_accumulate or its moments instance included, snapshots and statistics not). After every
step of the flagged session the statistic is evaluated (its own device_ms) and the NOISE
snapshot taken into device memory (host wall time around the call: tile-list copy, launch and
synchronise included, an upper bound of k_noise_resolve's time). Written to
<out>/noise_c3.json (default profiles/<name>/).

    python tools/noise_probe.py --name r13a

The kernels' own times come from a run of their own under the profiler, which this tool only
shortens (one round, no warm-up):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/noise_probe.py --name r13a --rounds 1 --warmup 0 --out DIR

Recorded, not judged: whether the moments instance costs more than k_accumulate's own
run-to-run spread is read off that trace.
"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, ".")
from izpi_amd import configs
from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer

ap = argparse.ArgumentParser()
ap.add_argument("--name", required=True, help="profiles/<name>/noise_c3.json")
ap.add_argument("--out", default=None, help="directory to write into instead of profiles/<name>")
ap.add_argument("--config", default="C3")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--step-spp", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()
cfg = configs.configs()[a.config]
total = a.steps * a.step_spp
r = GPURenderer(cfg.build(), cfg.width, cfg.height, total, max_depth=cfg.max_depth, sampler=cfg.sampler, device=0,
                bvh="gpu", accumulation=N.ACC_FORWARD)
import torch
snap = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
sessions = {"plain": [], "noise": []}
evaluations = []
for rnd in range(a.warmup + a.rounds):
    for name in ("plain", "noise"):
        t0 = time.perf_counter()
        evals = []
        with r.progressive(a.step_spp, noise=name == "noise") as s:
            while s.done < s.total:
                s.step()
                if name == "noise":
                    st = s.noise()
                    t1 = time.perf_counter()
                    s.snapshot_device(snap.data_ptr(), N.SNAP_NOISE)
                    evals.append({"done": st["done"], "stats_device_ms": round(st["device_ms"], 4),
                                  "snapshot_wall_us": round((time.perf_counter() - t1) * 1e6, 1), "above": st["above"],
                                  "pixels": st["pixels"], "nonfinite": st["nonfinite"], "max_error": st["max_error"],
                                  "mean_error": st["sum_error"] / max(1, st["pixels"] - st["nonfinite"])})
            st = s.stats
        wall_ms = (time.perf_counter() - t0) * 1e3
        if rnd >= a.warmup:
            sessions[name].append({"device_ms": round(st["total_ms"], 3), "wall_ms": round(wall_ms, 3),
                                   "trace_ms": round(st["kernel_ms"], 3), "shade_ms": round(st["shade_ms"], 3),
                                   "rays": st["rays"], "chunk_spp": st["chunk_spp"],
                                   "workspace_gb": round(st["workspace_bytes"] / 1e9, 3)})
            if name == "noise":
                evaluations.append(evals)
        print("probe: round %d %s %.1f ms device" % (rnd, name, st["total_ms"]), file=sys.stderr, flush=True)
r.close()
assert len({f["rays"] for v in sessions.values() for f in v}) == 1  # the flag changes no ray

med = {k: statistics.median(f["device_ms"] for f in v) for k, v in sessions.items()}
spread = {k: round(max(f["device_ms"] for f in v) - min(f["device_ms"] for f in v), 3) for k, v in sessions.items()}
out = {"config": cfg.name, "width": cfg.width, "height": cfg.height, "steps": a.steps, "step_spp": a.step_spp, "bvh": "gpu",
       "accumulation": "forward", "sessions": sessions, "median_device_ms": med, "spread_device_ms": spread,
       "noise_over_plain_ms": round(med["noise"] - med["plain"], 3), "evaluations": evaluations}
path = Path(a.out) if a.out else Path("profiles") / a.name
path.mkdir(parents=True, exist_ok=True)
(path / "noise_c3.json").write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps({"median_device_ms": med, "spread_device_ms": spread, "noise_over_plain_ms": out["noise_over_plain_ms"],
                  "last_evaluation": evaluations[-1][-1] if evaluations else None}))
